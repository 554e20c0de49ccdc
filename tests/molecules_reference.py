"""The molecule counter's contract (include/sctools_hip.h, "counting molecules") restated in plain
Python: a set of (index, umi) tuples, lists for reads and molecules, and a bad-UMI test written
triplet by triplet.  The device counter, its key header and the Python class are compared with this
module by exact equality."""


def idx_bits(nw):
    return max(1, (nw - 1).bit_length())


def check_params(nw, kind, L):
    """umi_bits of a legal counter; ValueError for what sct_molecules_create rejects."""
    if not 1 <= nw < 2 ** 31:
        raise ValueError("nw outside [1, 2^31)")
    if kind not in (2, 3):
        raise ValueError("kind must be 2 or 3")
    if L < 1:
        raise ValueError("L must be >= 1")
    if idx_bits(nw) + kind * L > 63:
        raise ValueError("index bits + UMI bits exceed 63")
    return kind * L


def umi_is_bad(umi, kind, L):
    """A bit at or above kind * L; for kind 3 also any of the L triplets that is not C 1, A 2, G 3
    or T 4 (N = 6, the invalid 0 / 5 / 7, a zero leading triplet)."""
    if umi >> (kind * L):
        return True
    if kind == 3:
        for p in range(L):
            if (umi >> (3 * p)) & 7 not in (1, 2, 3, 4):
                return True
    return False


def key(index, umi, kind, L):
    return (index << (kind * L)) | umi


class Molecules:
    def __init__(self, nw, kind, L):
        check_params(nw, kind, L)
        self.nw, self.kind, self.L = nw, kind, L
        self.reads = [0] * nw
        self.molecules = [0] * nw
        self.tally = [0, 0, 0]  # no match, ambiguous, bad UMI
        self.seen = set()
        self.total = 0

    def update(self, index, umis):
        """Counts every read; raises ValueError afterwards if an index lay outside [-2, nw)."""
        index, umis = [int(i) for i in index], [int(u) for u in umis]
        if len(index) != len(umis):
            raise ValueError("index and umis differ in length")
        out_of_range = False
        for i, u in zip(index, umis):
            self.total += 1
            if i == -1:
                self.tally[0] += 1
            elif i == -2:
                self.tally[1] += 1
            elif i < -2 or i >= self.nw:
                out_of_range = True
            elif umi_is_bad(u, self.kind, self.L):
                self.tally[2] += 1
            else:
                self.reads[i] += 1
                if (i, u) not in self.seen:
                    self.seen.add((i, u))
                    self.molecules[i] += 1
        if out_of_range:
            raise ValueError("index outside [-2, %d)" % self.nw)
        return self

    def counts(self):
        return list(self.reads), list(self.molecules), self.tally[0], self.tally[1], self.tally[2]

    def pairs(self):
        return sorted(self.seen)

    def saturation(self):
        total = sum(self.reads)
        return 1.0 - sum(self.molecules) / total if total else float("nan")
