"""Brute-force reference of posterior barcode correction (include/sctools_hip.h,
sct_nearest_correct), in Python ints over the whole whitelist.  It imports nothing from the
package under test: the contract is applied literally, digit by digit.

Codes: kind 2 is TwoBit (A 0, C 1, T 2, G 3), kind 3 ThreeBit (C 1, A 2, G 3, T 4, N 6), the first
base in the highest of the L digits.  Quality row byte b belongs to base b, digit L - 1 - b.
"""

TWO = {"A": 0, "C": 1, "T": 2, "G": 3}
THREE = {"C": 1, "A": 2, "G": 3, "T": 4, "N": 6}


def encode(kind, seq):
    """The code of a base string (kind 3 also takes 'N'; a digit 0..7 stands for that raw triplet)."""
    table = TWO if kind == 2 else THREE
    code = 0
    for ch in seq:
        code = (code << kind) | (int(ch) if ch.isdigit() else table[ch])
    return code


def digits(code, kind, L):
    """digit i of the code (base L - 1 - i), i = 0 .. L - 1"""
    mask = (1 << kind) - 1
    return [(code >> (kind * i)) & mask for i in range(L)]


def distance(kind, a, b):
    """the reference's hamming_distance: the kind-bit groups of a ^ b that are not zero"""
    x, d, mask = a ^ b, 0, (1 << kind) - 1
    while x:
        d += (x & mask) != 0
        x >>= kind
    return d


def _one_off_digit(kind, x):
    """-1 if x = a ^ b has no or several non-zero groups, else the digit of its only one"""
    mask = (1 << kind) - 1
    found, i = -1, 0
    while x:
        if x & mask:
            if found >= 0:
                return -1
            found = i
        x >>= kind
        i += 1
    return found


def scan(kind, L, whitelist, queries):
    """Per query, before any prior: ('high',) for bits at or above kind * L, ('exact', [indices at
    distance 0]) or ('near', [(index, differing digit) at distance 1])."""
    wl = [int(w) for w in whitelist]
    out = []
    for q in queries:
        q = int(q)
        if q >> (kind * L):
            out.append(("high",))
            continue
        exact = [j for j, w in enumerate(wl) if w == q]
        if exact:
            out.append(("exact", exact))
            continue
        near = []
        for j, w in enumerate(wl):
            i = _one_off_digit(kind, q ^ w)
            if i >= 0:
                assert distance(kind, q, w) == 1
                near.append((j, i))
        out.append(("near", near))
    return out


def decide(L, scanned, quals, prior, qweight, num, den):
    """(index list, dist list) from scan()'s rows: rules 1-5 of the contract."""
    assert 1 <= num <= den <= 64 and 2 * num > den
    index, dist = [], []
    for row, qual in zip(scanned, quals):
        if row[0] == "high":
            index.append(-1), dist.append(255)
        elif row[0] == "exact":
            index.append(row[1][0] if len(row[1]) == 1 else -2), dist.append(0)
        else:
            scores = []
            for j, i in row[1]:
                p = 1 if prior is None else int(prior[j])
                if p > 0:
                    scores.append((p * int(qweight[int(qual[L - 1 - i])]), j))
            if not scores:
                index.append(-1), dist.append(255)
                continue
            total = sum(s for s, _ in scores)
            best, jbest = max(scores)
            assert total < 1 << 56
            index.append(jbest if den * best >= num * total else -2), dist.append(1)
    return index, dist


def correct(kind, L, whitelist, queries, quals, prior, qweight, num, den):
    return decide(L, scan(kind, L, whitelist, queries), quals, prior, qweight, num, den)


def phred_weights(offset=33, cap=33):
    """round(2^20 * 10^(-Q/10)), Q = min(max(b - offset, 0), cap), in exact decimal arithmetic"""
    from decimal import Decimal, getcontext, ROUND_HALF_EVEN
    getcontext().prec = 50
    out = []
    for b in range(256):
        q = min(max(b - offset, 0), cap)
        v = Decimal(1 << 20) * (Decimal(10) ** (Decimal(-q) / Decimal(10)))
        out.append(int(v.to_integral_value(rounding=ROUND_HALF_EVEN)))
    return out
