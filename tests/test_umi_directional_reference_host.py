"""CPU: tests/umi_directional_reference.py against itself and against the one-step reference.  The
root of a molecule is stated twice there, as the fixpoint the device runs and as UMI-tools'
sequential procedure; here the two are shown equal on random small sets, the number of clusters is
shown not to depend on how ties among equal reads are broken, and the hand cases of the contract are
worked through.  The method-name function of sctools_amd.counting is checked as well."""

import random

import pytest

import umi_collapse_reference as U
import umi_directional_reference as D

C, A, G, T = 1, 2, 3, 4


def umi3(*bases):
    code = 0
    for b in bases:
        code = (code << 3) | b
    return code


def _random_set(rng, kind, L, n, nw=2):
    """n reads over a few UMIs near each other: a handful of seeds, their one-base neighbours and
    neighbours' neighbours, with reads drawn so that 1-read sets, equal reads and 2a - 1 all occur."""
    lo = 1 if kind == 3 else 0
    pool = []
    for _ in range(rng.randint(1, 3)):
        u = sum(rng.randint(lo, lo + 3) << (kind * p) for p in range(L))
        near = [u] + U.neighbours(u, kind, L)
        near += [w for v in rng.sample(near, min(3, len(near))) for w in U.neighbours(v, kind, L)]
        pool += near
    ref = D.DirectionalMolecules(nw, kind, L)
    for _ in range(n):
        k = rng.choice((1, 1, 1, 2, 3, 5))
        ref.update([rng.randrange(nw)] * k, [rng.choice(pool)] * k)
    return ref


def _sets():
    rng = random.Random(20)
    out = []
    for kind in (2, 3):
        for L in (1, 2, 3, 4, 5):
            for n in (1, 2, 4, 8, 16, 40):
                for _ in range(5):
                    out.append(_random_set(rng, kind, L, n))
    return out


SETS = _sets()


def _per_barcode(ref, root):
    per = D.clusters(root)
    return [per.get(i, 0) for i in range(ref.nw)]


def _every_pair_joined(ref):
    """No edge fails the threshold: any two stored UMIs one base apart are joined from the better to
    the lesser."""
    for (i, v), rv in ref.mreads.items():
        for u in U.neighbours(v, ref.kind, ref.L):
            if (i, u) in ref.mreads and U.support_less(rv, v, ref.mreads[(i, u)], u) and not D.edge(ref.mreads[(i, u)], rv):
                return False
    return True


def _no_grandparents(ref):
    """No two edges a -> b -> c with a != c."""
    for (i, c) in ref.mreads:
        for b in D.in_neighbours(ref.mreads, ref.kind, ref.L, i, c):
            if any(a != c for a in D.in_neighbours(ref.mreads, ref.kind, ref.L, i, b)):
                return False
    return True


def test_update_counts_what_the_one_step_reference_counts():
    ref = SETS[-1]
    assert isinstance(ref, U.CountedMolecules) and sum(ref.mreads.values()) == sum(ref.reads)


def test_the_sequential_procedure_equals_the_fixpoint():
    rounds = 0
    for ref in SETS:
        fix, n = D.fixpoint_roots(ref.mreads, ref.kind, ref.L)
        assert D.greedy_roots(ref.mreads, ref.kind, ref.L) == fix
        assert ref.collapse_directional() == (_per_barcode(ref, fix), sum(r != v for (_, v), r in fix.items()))
        rounds = max(rounds, n)
    assert rounds >= 2  # some set needed the transitive part


def test_cluster_counts_do_not_depend_on_the_tie_order():
    """UMI-tools orders equal reads by insertion, the contract by code: whatever the order among
    equals, the number of clusters per barcode is the same (the roots' names may differ)."""
    rng = random.Random(21)
    renamed = 0
    for ref in SETS:
        want = D.fixpoint_roots(ref.mreads, ref.kind, ref.L)[0]
        for _ in range(4):
            keys = list(ref.mreads)
            rng.shuffle(keys)
            got = D.greedy_roots(ref.mreads, ref.kind, ref.L, rank={k: n for n, k in enumerate(keys)})
            assert _per_barcode(ref, got) == _per_barcode(ref, want)
            assert all(ref.mreads[(i, r)] == ref.mreads[(i, want[(i, v)])] for (i, v), r in got.items())
            renamed += got != want
    assert renamed >= 10  # the shuffles did change roots' names


def test_against_the_one_step_rule():
    """Where every two stored neighbours are joined, a directional root has no better neighbour, so
    it is a one-step root: clusters <= one-step roots.  (Without that condition it does not hold:
    4 and 4 reads one base apart are two clusters and one one-step root.)  Where in addition no
    molecule has a grandparent, root and one-step parent are the same UMI for every molecule:
    clusters == one-step collapsed."""
    joined = flat = fewer = 0
    for ref in SETS:
        clusters = ref.collapse_directional()[0]
        if not _every_pair_joined(ref):
            continue
        joined += 1
        assert all(c <= r for c, r in zip(clusters, ref.roots()))
        fewer += clusters != ref.roots()
        if _no_grandparents(ref):
            flat += 1
            assert clusters == ref.collapse()[0]
            assert [r[3] for r in ref.pairs_directional()] == [r[3] for r in ref.pairs_counted()]
    assert joined >= 50 and flat >= 20 and fewer >= 3, (joined, flat, fewer)
    pair = D.DirectionalMolecules(1, 3, 2).update([0] * 8, [umi3(A, C)] * 4 + [umi3(A, G)] * 4)
    assert pair.collapse_directional() == ([2], 0) and pair.roots() == [1]


def _one(kind, L, reads):
    ref = D.DirectionalMolecules(1, kind, L)
    return ref.update([0] * len(reads), reads)


def test_hand_cases():
    # the header's chain: one molecule with two errors
    chain = _one(3, 2, [umi3(A, A)] + [umi3(A, C)] * 2 + [umi3(G, C)] * 5)
    assert chain.collapse() == ([2], 2) and chain.collapse_directional() == ([1], 2)
    assert [r[3] for r in chain.pairs_directional()] == [umi3(G, C)] * 3
    # the threshold: 3 over 2 is joined, 2 and 2 are not, 4 and 4 are not
    assert _one(3, 2, [umi3(A, C)] * 3 + [umi3(A, G)] * 2).collapse_directional() == ([1], 1)
    for n in (2, 4):
        equal = _one(3, 2, [umi3(A, C)] * n + [umi3(A, G)] * n)
        assert equal.collapse_directional() == ([2], 0) and equal.collapse() == ([1], 1)
    assert D.edge(1, 1) and D.edge(3, 2) and not D.edge(2, 2) and D.edge(5, 3) and not D.edge(4, 3)
    # the best ancestor comes through the lesser parent: v x 1, p1 x 10, p2 x 8, g x 100 beside p2 only
    v, p1, p2, g = umi3(A, A, A), umi3(A, A, C), umi3(A, C, A), umi3(G, C, A)
    anc = _one(3, 3, [v] + [p1] * 10 + [p2] * 8 + [g] * 100)
    root = anc.directional_roots()
    assert anc.parent(0, v) == p1 and root[(0, v)] == g and root[(0, p1)] == p1 and root[(0, p2)] == g
    assert anc.collapse_directional() == ([2], 2)
    # three 1-read UMIs pairwise one base apart: one cluster, named by the largest code
    three = _one(3, 2, [umi3(A, C), umi3(A, A), umi3(A, T)])
    assert three.collapse_directional() == ([1], 2) and set(three.directional_roots().values()) == {umi3(A, T)}
    # L = 1, both encodings; nothing at all
    assert _one(3, 1, [C, A, A, A, G]).collapse_directional() == ([1], 2)
    assert _one(2, 1, [0, 3]).collapse_directional() == ([1], 1)
    assert _one(2, 1, [0, 0, 3, 3]).collapse_directional() == ([2], 0)
    empty = D.DirectionalMolecules(3, 3, 2)
    assert empty.collapse_directional() == ([0, 0, 0], 0) and empty.saturation_directional() != empty.saturation_directional()


def test_a_long_path_needs_many_rounds():
    """100 one-read UMIs, each one base from the next and from no other: one cluster, and the plain
    fixpoint takes about as many rounds as the path is long."""
    L = 10
    path = D.snake(3, L, 100, random.Random(22))
    assert len(set(path)) == 100 and all(b in U.neighbours(a, 3, L) for a, b in zip(path, path[1:]))
    ref = D.DirectionalMolecules(2, 3, L).update([0] * 100 + [1] * 100, path + path)
    assert ref.collapse_directional() == ([1, 1], 198)
    assert D.fixpoint_roots(ref.mreads, 3, L)[1] >= 50
    assert D.greedy_roots(ref.mreads, 3, L) == ref.directional_roots()


def test_method_names():
    from sctools_amd import _lib, counting
    assert counting.collapse_method("one_step") == _lib.COLLAPSE_ONE_STEP == 0
    assert counting.collapse_method("directional") == _lib.COLLAPSE_DIRECTIONAL == 1
    for bad in ("Directional", "adjacency", "cluster", "", None, 1, 0, b"directional"):
        with pytest.raises(ValueError):
            counting.collapse_method(bad)
