"""The feature counter's contract (include/sctools_hip.h, "counting molecules per feature") restated
in plain Python on top of molecules_reference and umi_collapse_reference: a dict of reads per
(index, feature, umi), the rules of a read written one after the other, and the CSR matrix built by
walking the sorted dict.  The device counter, its key header and the Python class are compared with
this module by exact equality."""

import molecules_reference as R
import umi_collapse_reference as U


def feat_bits(nf):
    return max(1, (nf - 1).bit_length())


def check_params(nw, nf, kind, L):
    """umi_bits of a legal feature counter; ValueError for what sct_molecules_create_features rejects."""
    umi_bits = R.check_params(nw, kind, L)
    if not 1 <= nf < 2 ** 31:
        raise ValueError("nf outside [1, 2^31)")
    if R.idx_bits(nw) + feat_bits(nf) + umi_bits > 63:
        raise ValueError("index bits + feature bits + UMI bits exceed 63")
    return umi_bits


def key(index, feature, umi, nf, kind, L):
    return (((index << feat_bits(nf)) | feature) << (kind * L)) | umi


def unkey(k, nf, kind, L):
    umi_bits, fb = kind * L, feat_bits(nf)
    return k >> (umi_bits + fb), (k >> umi_bits) & ((1 << fb) - 1), k & ((1 << umi_bits) - 1)


class FeatureMolecules:
    def __init__(self, nw, nf, kind, L):
        check_params(nw, nf, kind, L)
        self.nw, self.nf, self.kind, self.L = nw, nf, kind, L
        self.reads = [0] * nw
        self.molecules = [0] * nw
        self.tally = [0, 0, 0, 0]  # no match, ambiguous, bad UMI, no feature
        self.mreads = {}  # (index, feature, umi) -> rule-5 reads
        self.total = 0

    def update(self, index, umis, features):
        """Counts every read; raises ValueError afterwards if an index lay outside [-2, nw) or a
        feature outside [-2, nf)."""
        index, umis, features = [int(i) for i in index], [int(u) for u in umis], [int(f) for f in features]
        if not len(index) == len(umis) == len(features):
            raise ValueError("index, umis and features differ in length")
        out_of_range = False
        for i, u, f in zip(index, umis, features):
            self.total += 1
            if i == -1:
                self.tally[0] += 1
            elif i == -2:
                self.tally[1] += 1
            elif i < -2 or i >= self.nw:
                out_of_range = True
            elif f < -2 or f >= self.nf:
                out_of_range = True
            elif R.umi_is_bad(u, self.kind, self.L):
                self.tally[2] += 1
            elif f < 0:
                self.tally[3] += 1
            else:
                self.reads[i] += 1
                if (i, f, u) not in self.mreads:
                    self.mreads[(i, f, u)] = 0
                    self.molecules[i] += 1
                self.mreads[(i, f, u)] += 1
        if out_of_range:
            raise ValueError("index outside [-2, %d) or feature outside [-2, %d)" % (self.nw, self.nf))
        return self

    def merge(self, other):
        for k, r in other.mreads.items():
            if k not in self.mreads:
                self.mreads[k] = 0
                self.molecules[k[0]] += 1
            self.mreads[k] += r
        self.reads = [a + b for a, b in zip(self.reads, other.reads)]
        self.tally = [a + b for a, b in zip(self.tally, other.tally)]
        self.total += other.total
        return self

    def counts(self):
        """What MoleculeCounter.counts() gives: three tallies."""
        return list(self.reads), list(self.molecules), self.tally[0], self.tally[1], self.tally[2]

    @property
    def n_no_feature(self):
        return self.tally[3]

    def parent(self, i, f, u):
        best = u
        for v in U.neighbours(u, self.kind, self.L):
            if (i, f, v) in self.mreads and U.support_less(self.mreads[(i, f, best)], best, self.mreads[(i, f, v)], v):
                best = v
        return best

    def pairs(self):
        """[(index, feature, umi, reads, parent umi)] in ascending key order."""
        return [(i, f, u, self.mreads[(i, f, u)], self.parent(i, f, u)) for (i, f, u) in sorted(self.mreads)]

    def collapse(self):
        """(collapsed per barcode, n_corrected)."""
        images, n_corrected = set(), 0
        for (i, f, u) in self.mreads:
            p = self.parent(i, f, u)
            images.add((i, f, p))
            n_corrected += p != u
        collapsed = [0] * self.nw
        for i, _, _ in images:
            collapsed[i] += 1
        return collapsed, n_corrected

    def matrix(self):
        """(indptr, feature, molecules, reads, collapsed) as lists: CSR over nw rows."""
        entries = {}  # (index, feature) -> [molecules, reads, set of parents]
        for (i, f, u), r in self.mreads.items():
            e = entries.setdefault((i, f), [0, 0, set()])
            e[0] += 1
            e[1] += r
            e[2].add(self.parent(i, f, u))
        order = sorted(entries)
        indptr = [0] * (self.nw + 1)
        for i, _ in order:
            indptr[i + 1] += 1
        for i in range(self.nw):
            indptr[i + 1] += indptr[i]
        return (indptr, [f for _, f in order], [entries[k][0] for k in order], [entries[k][1] for k in order],
                [len(entries[k][2]) for k in order])
