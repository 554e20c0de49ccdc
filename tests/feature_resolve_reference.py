"""Resolving features (include/sctools_hip.h, "resolving features") restated in plain Python on top
of count_matrix_reference and umi_directional_reference.  This module is the contract: the device
counter, the key header's fold and the Python class are compared with it by exact equality.

A row is (index, feature, umi, reads, image umi): a stored key, its reads and the UMI it collapses
into under its own (index, feature) -- itself ('none'), its one-step parent ('one_step',
FeatureMolecules.pairs()) or its directional root ('directional', feature_answers(fm)[2]; the roots
follow this project's tie rule, the larger code, not UMI-tools' insertion order).

A collapsed molecule is (index, feature, image) with the summed reads of its rows.  A group is the
collapsed molecules that share (index, image) over all features.  With top the largest reads of a
group: exactly one member at top is kept and the others are lost; two or more at top tie every
member of the group, the ones below top included."""

import umi_directional_reference as D

METHODS = ("none", "one_step", "directional")


def rows_from_dict(mreads):
    """The rows of a raw {(index, feature, umi): reads} dict with every key its own image."""
    return [(i, f, u, r, u) for (i, f, u), r in sorted(mreads.items())]


def rows_of(fm, method):
    """The rows of a count_matrix_reference.FeatureMolecules under a method's images."""
    if method == "none":
        return rows_from_dict(fm.mreads)
    if method == "one_step":
        return fm.pairs()
    if method == "directional":
        return D.feature_answers(fm)[2]
    raise ValueError("method must be one of %r" % (METHODS,))


def collapsed_molecules(rows):
    """{(index, feature, image): reads}: the np.unique recipe of the README."""
    out = {}
    for i, f, _, r, image in rows:
        out[(i, f, image)] = out.get((i, f, image), 0) + r
    return out


def fold(reads):
    """(top, members at top capped at 2, members, reads) of a list of member reads: the state the
    device folds, molecules_resolve_key.h."""
    top = max(reads) if reads else 0
    return top, min(2, sum(r == top for r in reads)), len(reads), sum(reads)


def resolve(rows):
    """(kept, n_shared, n_lost, n_tied, reads_dropped): kept is the set of (index, feature, image)
    that keep their molecule."""
    groups = {}
    for (i, f, image), r in collapsed_molecules(rows).items():
        groups.setdefault((i, image), []).append((f, r))
    kept, n_shared, n_lost, n_tied, dropped = set(), 0, 0, 0, 0
    for (i, image), members in groups.items():
        top = max(r for _, r in members)
        at_top = [f for f, r in members if r == top]
        n_shared += len(members) >= 2
        if len(at_top) == 1:
            kept.add((i, at_top[0], image))
            n_lost += len(members) - 1
            dropped += sum(r for _, r in members) - top
        else:
            n_tied += len(members)
            dropped += sum(r for _, r in members)
    return kept, n_shared, n_lost, n_tied, dropped


def group_kinds(rows):
    """(groups of one member, groups of several with a unique winner, tied groups): what a test's
    input must hold of each before it says anything about the device."""
    groups = {}
    for (i, _, image), r in collapsed_molecules(rows).items():
        groups.setdefault((i, image), []).append(r)
    alone = sum(len(m) == 1 for m in groups.values())
    tied = sum(fold(m)[1] == 2 for m in groups.values())
    return alone, len(groups) - alone - tied, tied


def mix(seed, n=6000, nw=5, nf=6, kind=3, L=6, hop=0.08, err=0.05, planted=8):
    """(index, feature, umi) lists of about n reads: molecules whose feature is a function of
    (barcode, UMI) with 1 to 12 reads each, a share `hop` of the reads moved to another feature drawn
    uniformly and a share `err` of them with one base of the UMI changed.  Then `planted` pairs: a UMI
    that is not stored and has no stored neighbour under its barcode, under two features with equal
    reads -- a tie under every method.  rng is random.Random(seed)."""
    import random

    import umi_collapse_reference as U

    rng = random.Random(seed)
    lo = 1 if kind == 3 else 0
    index, feature, umi = [], [], []
    while len(index) < n:
        i = rng.randrange(nw)
        u = sum(rng.randrange(lo, lo + 4) << (kind * p) for p in range(L))
        f = (i * 7 + u * 13) % nf
        for _ in range(rng.randrange(1, 13)):
            ff = f if rng.random() >= hop else rng.choice([x for x in range(nf) if x != f])
            uu = u if rng.random() >= err else rng.choice(U.neighbours(u, kind, L))
            index.append(i), feature.append(ff), umi.append(uu)
    stored = {(i, u) for i, u in zip(index, umi)}
    done = 0
    while done < planted:
        i = rng.randrange(nw)
        u = sum(rng.randrange(lo, lo + 4) << (kind * p) for p in range(L))
        if (i, u) in stored or any((i, v) in stored for v in U.neighbours(u, kind, L)):
            continue
        stored.add((i, u))
        f1, f2 = rng.sample(range(nf), 2)
        reads = rng.randrange(1, 5)
        index += [i] * (2 * reads)
        feature += [f1, f2] * reads
        umi += [u] * (2 * reads)
        done += 1
    return index, feature, umi


def answer(fm, method):
    """What MoleculeCounter.resolve(method) gives: (resolved per barcode as a list of nw, n_shared,
    n_lost, n_tied, reads_dropped)."""
    kept, n_shared, n_lost, n_tied, dropped = resolve(rows_of(fm, method))
    per = [0] * fm.nw
    for i, _, _ in kept:
        per[i] += 1
    return per, n_shared, n_lost, n_tied, dropped


def matrix_resolved(fm, method):
    """(indptr, feature, molecules, reads, collapsed, resolved) as lists: the matrix of
    FeatureMolecules.matrix() with the method's collapsed column (None for 'none') and the kept
    molecules of every entry after it -- an entry that keeps nothing holds 0."""
    indptr, feature, molecules, reads, one_step = fm.matrix()
    collapsed = {"none": None, "one_step": one_step}.get(method)
    if method == "directional":
        collapsed = D.feature_answers(fm)[3]
    per = {}
    for i, f, _ in resolve(rows_of(fm, method))[0]:
        per[(i, f)] = per.get((i, f), 0) + 1
    entries = [(i, f) for i in range(fm.nw) for f in feature[indptr[i]:indptr[i + 1]]]
    return indptr, feature, molecules, reads, collapsed, [per.get(e, 0) for e in entries]
