"""CPU: tests/read_groups_reference.py, the read-groups contract in plain Python, on the cases worked
by hand (the expected tuples are written out in tests/read_groups_cases.py) and, on
feature_resolve_reference.mix, the three invariants that tie the per-read answers to the counter's own
totals.  Every comparison is exact equality."""

import pytest

import feature_resolve_reference as F
import read_groups_cases as C
import read_groups_reference as G
import umi_directional_reference as D


@pytest.mark.parametrize("kind", [3, 2])
@pytest.mark.parametrize("name", ["worked", "kept_and_lost", "tied", "alone"])
def test_feature_cases_worked_by_hand(kind, name):
    nw, nf, mreads, batch, expected = C.feature_cases(kind)[name]
    fm = C.feature_reference(nw, nf, kind, 3, mreads)
    index, feature, umi = zip(*batch)
    for method in F.METHODS:
        for resolved in (False, True):
            want = C.expected_of(expected, method, resolved)
            assert want is not None and len(want) == len(batch)
            groups = G.ReadGroups(fm, method, resolved)
            assert groups.tag(index, umi, feature) == C.columns(want), (method, resolved)
            assert groups.tagged == len(batch)


@pytest.mark.parametrize("kind", [3, 2])
def test_plain_case_worked_by_hand(kind):
    nw, mreads, batch, expected = C.plain_cases(kind)["worked"]
    cm = C.plain_reference(nw, kind, 3, mreads)
    index, umi = zip(*batch)
    for method in F.METHODS:
        assert G.ReadGroups(cm, method).tag(index, umi) == C.columns(expected[method]), method
    with pytest.raises(ValueError):
        G.ReadGroups(cm, "none", resolved=True)


def test_first_runs_across_calls_and_a_bad_index_still_tags_the_batch():
    nw, nf, mreads, batch, expected = C.feature_cases(3)["kept_and_lost"]
    fm = C.feature_reference(nw, nf, 3, 3, mreads)
    want = C.columns(C.expected_of(expected, "none", False))
    groups = G.ReadGroups(fm, "none")
    index, feature, umi = zip(*batch)
    pieces = [groups.tag(index[:1], umi[:1], feature[:1]), groups.tag(index[1:], umi[1:], feature[1:])]
    assert tuple(a + b for a, b in zip(*pieces)) == want
    with pytest.raises(ValueError):
        groups.tag([nw, 1, 1], [umi[0]] * 3, [0, nf, 0])
    assert groups.last == ([umi[0]] * 3, [G.BAD_INDEX, G.BAD_INDEX, G.GROUPED], [0, 0, 5], [False] * 3)
    assert groups.tagged == len(batch) + 3
    assert groups.tally == [5, 0, 0, 0, 0, 0, 0, 2]


def test_a_snapshot_does_not_see_later_updates():
    nw, nf, mreads, batch, _ = C.feature_cases(3)["alone"]
    fm = C.feature_reference(nw, nf, 3, 3, mreads)
    groups = G.ReadGroups(fm, "none")
    fm.update([0], [batch[3][2]], [1])  # the batch's first absent key is stored now
    assert groups.tag(*[[b[k] for b in batch] for k in (0, 2, 1)])[1][3] == G.ABSENT
    assert G.ReadGroups(fm, "none").tag(*[[b[k] for b in batch] for k in (0, 2, 1)])[1][3] == G.GROUPED


@pytest.mark.parametrize("kind", [3, 2])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_invariants_on_mix(seed, kind):
    """When every counted read is tagged exactly once: count(first) is the molecules the method (and
    resolve) leaves, count(LOST) is reads_dropped, and the first reads' molecules carry every read
    that was not dropped."""
    fm, batch = C.mix_case(seed, kind)
    index, feature, umi = batch
    collapsed = {"none": sum(fm.molecules), "one_step": sum(fm.collapse()[0]),
                 "directional": sum(D.feature_answers(fm)[0])}
    for method in F.METHODS:
        resolved_per, _, _, _, reads_dropped = F.answer(fm, method)
        for resolved in (False, True):
            C.assert_input_holds(fm, batch, method, resolved)
            final, status, mol_reads, first = G.ReadGroups(fm, method, resolved).tag(index, umi, feature)
            dropped = reads_dropped if resolved else 0
            assert sum(first) == (sum(resolved_per) if resolved else collapsed[method])
            assert status.count(G.LOST) == dropped
            assert sum(r for r, f in zip(mol_reads, first) if f) + dropped == sum(fm.reads)
            assert all(s == G.GROUPED for s, f in zip(status, first) if f)
            # the UMI changes only where a stored key has another image, and never for statuses 1..5
            assert all(a == b for a, b, s in zip(final, umi, status) if s not in (G.GROUPED, G.LOST))
            if method == "none":
                assert final == umi
            else:
                assert sum(a != b for a, b in zip(final, umi)) > 180
            if resolved:
                assert status.count(G.LOST) > 240
