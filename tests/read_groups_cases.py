"""Inputs shared by the read-groups tests (tests/test_read_groups_reference_host.py on the CPU,
tests/test_gpu_read_groups.py on the device): the cases worked by hand with their expected
(final_umi, status, mol_reads, first) tuples written out, and the tag batches made from
feature_resolve_reference.mix with planted reads of every status."""

import functools
import random

import count_matrix_reference as M
import feature_resolve_reference as F
import read_groups_reference as G
import umi_collapse_reference as U
import umi_directional_reference as D

GR, AB, LO = G.GROUPED, G.ABSENT, G.LOST


def umi_of(kind, *digits):
    """A good code of the digits 0..3, written first base first (the first base in the high digit)."""
    code = 0
    for d in digits:
        code = (code << kind) | (d + (1 if kind == 3 else 0))
    return code


def feature_reference(nw, nf, kind, L, mreads):
    """The FeatureMolecules that holds {(index, feature, umi): reads} (no read is walked)."""
    fm = M.FeatureMolecules(nw, nf, kind, L)
    fm.mreads = dict(mreads)
    for (i, _, _), r in mreads.items():
        fm.reads[i] += r
        fm.molecules[i] += 1
    fm.total = sum(mreads.values())
    return fm


def plain_reference(nw, kind, L, mreads):
    """The DirectionalMolecules that holds {(index, umi): reads}."""
    cm = D.DirectionalMolecules(nw, kind, L)
    cm.mreads = dict(mreads)
    cm.seen = set(mreads)
    for (i, _), r in mreads.items():
        cm.reads[i] += r
        cm.molecules[i] += 1
    cm.total = sum(mreads.values())
    return cm


def reads_of(mreads):
    """Every molecule's reads as a list of its key repeated, in key order."""
    return [k for k, r in sorted(mreads.items()) for _ in range(r)]


def feature_cases(kind):
    """{name: (nw, nf, mreads, tag batch [(index, feature, umi)], {(method, resolved): expected})}, L = 3.
    An expected list holds one (final_umi, status, mol_reads, first) per read of the batch; a key of
    ("any", resolved) stands for all three methods."""
    a, a2, u = umi_of(kind, 1, 1, 0), umi_of(kind, 1, 1, 2), umi_of(kind, 2, 3, 0)
    z, t = umi_of(kind, 0, 0, 0), umi_of(kind, 3, 3, 3)
    T, N = True, False
    # collapse turns a tie into a win: A x 1 and A' x 3 under feature 1, A' x 3 under feature 2
    worked_batch = [(0, 1, a2), (0, 2, a2), (0, 1, a), (0, 1, a2), (0, 2, a2), (0, 1, a2), (0, 2, a2)]
    collapsed = [(a2, GR, 4, T), (a2, GR, 3, T), (a2, GR, 4, N), (a2, GR, 4, N), (a2, GR, 3, N), (a2, GR, 4, N),
                 (a2, GR, 3, N)]
    collapsed_resolved = [(a2, GR, 4, T), (a2, LO, 3, N), (a2, GR, 4, N), (a2, GR, 4, N), (a2, LO, 3, N),
                          (a2, GR, 4, N), (a2, LO, 3, N)]
    return {
        "worked": (1, 3, {(0, 1, a): 1, (0, 1, a2): 3, (0, 2, a2): 3}, worked_batch, {
            ("none", False): [(a2, GR, 3, T), (a2, GR, 3, T), (a, GR, 1, T), (a2, GR, 3, N), (a2, GR, 3, N),
                              (a2, GR, 3, N), (a2, GR, 3, N)],
            ("none", True): [(a2, LO, 3, N), (a2, LO, 3, N), (a, GR, 1, T), (a2, LO, 3, N), (a2, LO, 3, N),
                             (a2, LO, 3, N), (a2, LO, 3, N)],
            ("one_step", False): collapsed, ("directional", False): collapsed,
            ("one_step", True): collapsed_resolved, ("directional", True): collapsed_resolved,
        }),
        "kept_and_lost": (2, 4, {(1, 0, u): 5, (1, 2, u): 3, (1, 3, u): 3},
                          [(1, 0, u), (1, 2, u), (1, 0, u), (1, 3, u)], {
            ("any", False): [(u, GR, 5, T), (u, GR, 3, T), (u, GR, 5, N), (u, GR, 3, T)],
            ("any", True): [(u, GR, 5, T), (u, LO, 3, N), (u, GR, 5, N), (u, LO, 3, N)],
        }),
        "tied": (2, 4, {(1, 0, u): 3, (1, 2, u): 3, (1, 3, u): 1}, [(1, 3, u), (1, 0, u), (1, 2, u), (1, 3, u)], {
            ("any", False): [(u, GR, 1, T), (u, GR, 3, T), (u, GR, 3, T), (u, GR, 1, N)],
            ("any", True): [(u, LO, 1, N), (u, LO, 3, N), (u, LO, 3, N), (u, LO, 1, N)],
        }),
        "alone": (2, 4, {(0, 3, z): 2, (1, 1, t): 1}, [(1, 1, t), (0, 3, z), (0, 3, z), (0, 1, z), (1, 1, z)], {
            ("any", False): [(t, GR, 1, T), (z, GR, 2, T), (z, GR, 2, N), (z, AB, 0, N), (z, AB, 0, N)],
            ("any", True): [(t, GR, 1, T), (z, GR, 2, T), (z, GR, 2, N), (z, AB, 0, N), (z, AB, 0, N)],
        }),
    }


def plain_cases(kind):
    """The same for a counter without features: {name: (nw, mreads, batch [(index, umi)], {method: expected})}.
    x is one base from both stored UMIs and not stored: ABSENT, never corrected."""
    a, a2, x = umi_of(kind, 1, 1, 0), umi_of(kind, 1, 1, 2), umi_of(kind, 1, 1, 3)
    T, N = True, False
    moved = [(a2, GR, 7, T), (a2, GR, 7, N), (a2, GR, 7, N), (x, AB, 0, N)]
    return {
        "worked": (1, {(0, a): 1, (0, a2): 6}, [(0, a), (0, a2), (0, a), (0, x)], {
            "none": [(a, GR, 1, T), (a2, GR, 6, T), (a, GR, 1, N), (x, AB, 0, N)],
            "one_step": moved, "directional": moved,
        }),
    }


def expected_of(expected, method, resolved):
    return expected.get((method, resolved), expected.get(("any", resolved)))


def columns(tuples):
    """[(final, status, reads, first)] as four lists."""
    return tuple([t[k] for t in tuples] for k in range(4))


@functools.lru_cache(maxsize=None)
def mix_case(seed, kind, nw=5, nf=6, L=6):
    """(fm, batch): the reference counter of F.mix(seed, n=3000, kind) and the tag batch -- the counted
    reads in a shuffled order with planted reads among them: indices -1 and -2, a UMI with N (ThreeBit)
    or a bit past its width (TwoBit) and, ThreeBit, an invalid zero triplet, a feature of -1 and of -2, a
    key that is not stored, and a key one base from a stored one that is not itself stored.  The batch is
    three lists (index, feature, umi)."""
    index, feature, umi = F.mix(seed, n=3000, nw=nw, nf=nf, kind=kind, L=L)
    fm = M.FeatureMolecules(nw, nf, kind, L).update(index, umi, feature)
    rng = random.Random(1000 + seed)
    reads = list(zip(index, feature, umi))
    rng.shuffle(reads)
    lo = 1 if kind == 3 else 0
    good = lambda: sum(rng.randrange(lo, lo + 4) << (kind * p) for p in range(L))  # noqa: E731
    stored = set(fm.mreads)
    planted = []
    for _ in range(5):
        planted.append((-1, rng.randrange(nf), good()))
        planted.append((-2, rng.randrange(nf), good()))
        bad = (good() & ~7) | 6 if kind == 3 else good() | (1 << (kind * L))
        planted.append((rng.randrange(nw), rng.randrange(nf), bad))
        if kind == 3:
            planted.append((rng.randrange(nw), rng.randrange(nf), good() & ~(7 << 3)))
        planted.append((rng.randrange(nw), -1, good()))
        planted.append((rng.randrange(nw), -2, good()))
        while True:  # not stored
            k = (rng.randrange(nw), rng.randrange(nf), good())
            if k not in stored:
                planted.append(k)
                break
        while True:  # one base from a stored key of the same barcode and feature, not stored
            i, f, u = rng.choice(reads)
            v = rng.choice(U.neighbours(u, kind, L))
            if (i, f, v) not in stored:
                planted.append((i, f, v))
                break
    for p in planted:
        reads.insert(rng.randrange(len(reads) + 1), p)
    return fm, tuple(list(col) for col in zip(*reads))


def assert_input_holds(fm, batch, method, resolved):
    """What an input must hold before anything is concluded from it, under `method`: a read of every
    status the flags allow, a molecule whose UMI moves (a collapsing method) and a group of each of
    feature_resolve_reference.group_kinds' three kinds."""
    rows = F.rows_of(fm, method)
    statuses = set(G.ReadGroups(fm, method, resolved).tag(batch[0], batch[2], batch[1])[1])
    assert statuses == set(range(7 if resolved else 6)), (method, resolved, sorted(statuses))
    if method != "none":
        assert G.moved(rows) >= 1, method
    alone, won, tied = F.group_kinds(rows)
    assert alone >= 1 and won >= 1 and tied >= 1, (method, alone, won, tied)
