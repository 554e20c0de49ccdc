"""The UMI collapse's contract (include/sctools_hip.h, "collapsing UMIs one base apart") restated in
plain Python on top of molecules_reference.Molecules: a dict of reads per (index, umi), the one-base
neighbours written digit by digit, the parent rule, and the collapse counted as the distinct parents
per barcode.  The device counter, the neighbour header and the Python class are compared with this
module by exact equality."""

import molecules_reference as R


def digits(umi, kind, L):
    """The L base values of a good UMI, low position first: 0..3 (kind 2) or 1..4 (kind 3)."""
    return [(umi >> (kind * p)) & (2 ** kind - 1) for p in range(L)]


def from_digits(ds, kind):
    return sum(d << (kind * p) for p, d in enumerate(ds))


def neighbours(umi, kind, L):
    """The 3 * L codes one base away from a good UMI: every position with each of the three other
    bases of its alphabet (0..3 for kind 2; 1..4 for kind 3: never N, never an invalid triplet)."""
    alphabet = (0, 1, 2, 3) if kind == 2 else (1, 2, 3, 4)
    ds = digits(umi, kind, L)
    out = []
    for p in range(L):
        for b in alphabet:
            if b != ds[p]:
                out.append(from_digits(ds[:p] + [b] + ds[p + 1:], kind))
    return out


def support_less(a_reads, a_code, b_reads, b_code):
    """(a_reads, a_code) < (b_reads, b_code): by reads, then by code."""
    return (a_reads, a_code) < (b_reads, b_code)


class CountedMolecules(R.Molecules):
    def __init__(self, nw, kind, L):
        super().__init__(nw, kind, L)
        self.mreads = {}  # (index, umi) -> rule-5 reads

    def update(self, index, umis):
        index, umis = [int(i) for i in index], [int(u) for u in umis]
        for i, u in zip(index, umis):
            if 0 <= i < self.nw and not R.umi_is_bad(u, self.kind, self.L):
                self.mreads[(i, u)] = self.mreads.get((i, u), 0) + 1
        return super().update(index, umis)

    def parent(self, i, u):
        best = u
        for v in neighbours(u, self.kind, self.L):
            if (i, v) in self.mreads and support_less(self.mreads[(i, best)], best, self.mreads[(i, v)], v):
                best = v
        return best

    def collapse(self):
        """(collapsed list of nw, n_corrected): distinct parents per barcode, molecules that move."""
        images = set()
        n_corrected = 0
        for (i, u) in self.mreads:
            p = self.parent(i, u)
            images.add((i, p))
            n_corrected += p != u
        collapsed = [0] * self.nw
        for i, _ in images:
            collapsed[i] += 1
        return collapsed, n_corrected

    def roots(self):
        """Molecules per barcode that are their own parent (what collapsed must NOT count)."""
        out = [0] * self.nw
        for (i, u) in self.mreads:
            out[i] += self.parent(i, u) == u
        return out

    def pairs_counted(self):
        """[(index, umi, reads, parent umi)] in ascending (index, umi) order."""
        return [(i, u, self.mreads[(i, u)], self.parent(i, u)) for (i, u) in sorted(self.mreads)]

    def saturation_collapsed(self):
        total = sum(self.reads)
        return 1.0 - sum(self.collapse()[0]) / total if total else float("nan")
