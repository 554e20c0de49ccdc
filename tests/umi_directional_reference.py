"""The directional clusters' contract (include/sctools_hip.h, "directional clusters") restated in
plain Python on top of umi_collapse_reference.CountedMolecules: the edge test as the big-integer
statement, the root of a molecule as the largest of everything that reaches it, and beside it
UMI-tools' sequential procedure, which the host test shows to give the same roots.  The device
counter and the Python class are compared with this module by exact equality.

The functions work on a dict of reads per (group, umi).  A group is whatever two related UMIs must
share: the index of a molecule counter, the (index, feature) pair of a feature counter.

UMI-tools breaks ties between molecules of equal reads by insertion order, this contract by code
(umi_collapse_reference.support_less).  Only the *name* of the root of mutually joined 1-read UMIs
can depend on that choice.  The number of clusters cannot: it is the number of strongly connected
components of the edge graph that no edge enters from outside, which `greedy_roots` with any
`rank` among equal reads reproduces (tests/test_umi_directional_reference_host.py shuffles it)."""

import umi_collapse_reference as U


def edge(u_reads, v_reads):
    """u -> v for two stored UMIs one base apart: reads(u) >= 2 * reads(v) - 1."""
    return u_reads >= 2 * v_reads - 1


def in_neighbours(mreads, kind, L, g, v):
    """The stored UMIs of group g with an edge into v."""
    return [u for u in U.neighbours(v, kind, L) if (g, u) in mreads and edge(mreads[(g, u)], mreads[(g, v)])]


def out_neighbours(mreads, kind, L, g, u):
    return [v for v in U.neighbours(u, kind, L) if (g, v) in mreads and edge(mreads[(g, u)], mreads[(g, v)])]


def fixpoint_roots(mreads, kind, L):
    """{(g, v): root umi}: the largest (reads, code) among v and everything that reaches v, found by
    repeating label[v] = max(label[v], label[a] over in-neighbours a) until nothing changes.  Also
    returns the number of rounds that changed something."""
    label = {(g, v): (r, v) for (g, v), r in mreads.items()}
    ins = {(g, v): in_neighbours(mreads, kind, L, g, v) for (g, v) in mreads}
    rounds = 0
    while True:
        new = {(g, v): max([label[(g, v)]] + [label[(g, a)] for a in ins[(g, v)]]) for (g, v) in mreads}
        if new == label:
            return {k: code for k, (_, code) in label.items()}, rounds
        label, rounds = new, rounds + 1


def greedy_roots(mreads, kind, L, rank=None):
    """UMI-tools' directional procedure: molecules in descending (reads, rank) order -- rank is the
    code unless given as {(g, umi): number} -- each one not yet claimed becomes a root and claims every
    unclaimed molecule reachable from it along edges.  {(g, v): root umi}."""
    rank = rank or {k: k[1] for k in mreads}
    root = {}
    for (g, u) in sorted(mreads, key=lambda k: (mreads[k], rank[k]), reverse=True):
        if (g, u) in root:
            continue
        root[(g, u)] = u
        stack = [u]
        while stack:
            a = stack.pop()
            for b in out_neighbours(mreads, kind, L, g, a):
                if (g, b) not in root:
                    root[(g, b)] = u
                    stack.append(b)
    return root


def clusters(root):
    """{group: number of roots} of a {(g, v): root} dict."""
    out = {}
    for (g, v), r in root.items():
        out[g] = out.get(g, 0) + (r == v)
    return out


def snake(kind, L, n, rng):
    """n distinct good UMIs, each one base from the next and from no other of them: a path in which
    an answer can only travel one step at a time.  rng is a random.Random."""
    lo = 1 if kind == 3 else 0
    path = [sum((lo + p % 4) << (kind * p) for p in range(L))]
    on_path = set(path)
    while len(path) < n:
        free = [v for v in U.neighbours(path[-1], kind, L)
                if v not in on_path and on_path.intersection(U.neighbours(v, kind, L)) == {path[-1]}]
        path.append(rng.choice(free))
        on_path.add(path[-1])
    return path


class DirectionalMolecules(U.CountedMolecules):
    """CountedMolecules with the directional answers beside the one-step ones."""

    def directional_roots(self):
        return fixpoint_roots(self.mreads, self.kind, self.L)[0]

    def collapse_directional(self):
        """(clusters per barcode as a list of nw, molecules with root != self)."""
        root = self.directional_roots()
        per = clusters(root)
        return [per.get(i, 0) for i in range(self.nw)], sum(r != v for (_, v), r in root.items())

    def pairs_directional(self):
        """[(index, umi, reads, root umi)] in ascending (index, umi) order."""
        root = self.directional_roots()
        return [(i, u, self.mreads[(i, u)], root[(i, u)]) for (i, u) in sorted(self.mreads)]

    def saturation_directional(self):
        total = sum(self.reads)
        return 1.0 - sum(self.collapse_directional()[0]) / total if total else float("nan")


def feature_answers(fm):
    """The directional answers of a count_matrix_reference.FeatureMolecules: (collapsed per barcode,
    n_corrected, [(index, feature, umi, reads, root umi)] in key order, clusters per matrix entry in
    entry order)."""
    grouped = {((i, f), u): r for (i, f, u), r in fm.mreads.items()}
    root = fixpoint_roots(grouped, fm.kind, fm.L)[0]
    per = clusters(root)
    collapsed = [0] * fm.nw
    for (i, _), n in per.items():
        collapsed[i] += n
    rows = [(i, f, u, fm.mreads[(i, f, u)], root[((i, f), u)]) for (i, f, u) in sorted(fm.mreads)]
    return collapsed, sum(r != v for (_, v), r in root.items()), rows, [per[e] for e in sorted(per)]
