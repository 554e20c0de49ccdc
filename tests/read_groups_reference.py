"""Read groups (include/sctools_hip.h, "read groups") restated in plain Python on top of
count_matrix_reference, umi_collapse_reference, umi_directional_reference and
feature_resolve_reference, whose rules are used and not restated.  This module is the contract: the
device tag kernels, the status header and the Python class are compared with it by exact equality.

A snapshot is made from a reference counter -- a count_matrix_reference.FeatureMolecules, or for a
counter without features an umi_directional_reference.DirectionalMolecules -- as it stands; later
updates of the counter do not reach it.  Its rows are feature_resolve_reference.rows_of's: (index,
feature, umi, reads, image umi), the feature None in a snapshot without features."""

import feature_resolve_reference as F
import molecules_reference as R
import umi_directional_reference as D

GROUPED, NO_BARCODE, AMBIGUOUS, BAD_UMI, NO_FEATURE, ABSENT, LOST, BAD_INDEX = range(8)
STATUS_NAMES = ("GROUPED", "NO_BARCODE", "AMBIGUOUS", "BAD_UMI", "NO_FEATURE", "ABSENT", "LOST", "BAD_INDEX")


def plain_rows(cm, method):
    """rows_of for a counter without features (a CountedMolecules or better; 'none' needs only
    Molecules.seen, and then every molecule's reads are 0: the snapshot has none to give)."""
    if method == "none":
        mreads = getattr(cm, "mreads", None)
        if mreads is None:
            return [(i, None, u, 0, u) for (i, u) in sorted(cm.seen)]
        return [(i, None, u, r, u) for (i, u), r in sorted(mreads.items())]
    if method == "one_step":
        return [(i, None, u, r, p) for i, u, r, p in cm.pairs_counted()]
    if method == "directional":
        root = D.fixpoint_roots(cm.mreads, cm.kind, cm.L)[0]
        return [(i, None, u, r, root[(i, u)]) for (i, u), r in sorted(cm.mreads.items())]
    raise ValueError("method must be one of %r" % (F.METHODS,))


class ReadGroups:
    def __init__(self, counter, method="one_step", resolved=False):
        self.nw, self.kind, self.L = counter.nw, counter.kind, counter.L
        self.nf = getattr(counter, "nf", None)
        if resolved and self.nf is None:
            raise ValueError("resolved=True needs a feature counter")
        self.rows = F.rows_of(counter, method) if self.nf is not None else plain_rows(counter, method)
        self.image = {(i, f, u): image for i, f, u, _, image in self.rows}
        self.reads = F.collapsed_molecules(self.rows)
        self.kept = F.resolve(self.rows)[0] if resolved else None
        self.tagged = 0
        self.first_seen = set()  # the final molecules that have had their first GROUPED read
        self.tally = [0] * 8

    def tag_one(self, i, f, u):
        """(final_umi, status, mol_reads, first) of the next read."""
        self.tagged += 1
        out = self._classify(i, f, u)
        self.tally[out[1]] += 1
        return out

    def _classify(self, i, f, u):
        if i == -1:
            return u, NO_BARCODE, 0, False
        if i == -2:
            return u, AMBIGUOUS, 0, False
        if i < -2 or i >= self.nw or (self.nf is not None and (f < -2 or f >= self.nf)):
            return u, BAD_INDEX, 0, False
        if R.umi_is_bad(u, self.kind, self.L):
            return u, BAD_UMI, 0, False
        if self.nf is not None and f < 0:
            return u, NO_FEATURE, 0, False
        if (i, f, u) not in self.image:
            return u, ABSENT, 0, False
        final = (i, f, self.image[(i, f, u)])
        if self.kept is not None and final not in self.kept:
            return final[2], LOST, self.reads[final], False
        first = final not in self.first_seen
        self.first_seen.add(final)
        return final[2], GROUPED, self.reads[final], first

    def tag(self, index, umis, features=None):
        """Four lists, one entry per read; raises ValueError afterwards if a read was BAD_INDEX."""
        if (features is None) != (self.nf is None):
            raise ValueError("features are given exactly to a feature counter's groups")
        index, umis = [int(i) for i in index], [int(u) for u in umis]
        features = [None] * len(index) if features is None else [int(f) for f in features]
        if not len(index) == len(umis) == len(features):
            raise ValueError("index, umis and features differ in length")
        out = [self.tag_one(i, f, u) for i, f, u in zip(index, features, umis)]
        self.last = tuple([o[k] for o in out] for k in range(4))
        if any(o[1] == BAD_INDEX for o in out):
            raise ValueError("index or feature out of range")
        return self.last


def moved(rows):
    """The stored keys whose image is another UMI."""
    return sum(u != image for _, _, u, _, image in rows)
