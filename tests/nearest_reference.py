"""The two fallback layouts of the nearest-whitelist index (sctools_amd/csrc/nearest.hip) restated
in Python integers, and inputs that put a whitelist on one seam of them.

Part 1, the mirror: the arithmetic nearest.hip documents -- the block split G*b/P*kind, the
open-addressing tables of pair keys (slot count the power of two >= max(4, 2 nw), the murmur
finalizer as the slot hash, groups of 4 slots probed linearly, the exact-hit shortcut over table
0's first group, the duplicate flag) and the CSR buckets per block (a provisional table of ~nw/2
buckets, then `load` buckets per occupied one, a multiplicative hash of the block's bits) -- with a
pure-Python build and query through each, and the reported size of the half-key tables.  The mirror
only chooses inputs and proves on the CPU that they reach a seam
(tests/test_nearest_reference_host.py); a GPU answer is never compared with it, only with the brute
force (oracle.c_nearest).  Each query takes `wrong`, the name of one
deliberately wrong variant: the host test shows that the seam inputs tell each from the brute force.

Part 2, the builders: (whitelist, queries, info) with uint64 arrays and what the mirror says the
input exercises.
"""

import numpy as np

M64 = (1 << 64) - 1
GROUP = 4  # slots per open-addressing group
MAX_KEYS = 6
MAX_PARTS = 8
GOLDEN = 0x9E3779B97F4A7C15

# the deliberately wrong variants (never built as kernels)
WRONG_OA = ("first_group_only", "no_wrap", "shortcut_ignores_dup", "drop_last_block", "no_tie")
WRONG_CSR = ("drop_last_block", "no_tie", "no_distance_check")


# ---------------------------------------------------------------- part 1: the mirror
def positions(kind, code_bits):
    return -(-code_bits // kind)


def dist(kind, a, b):
    x = a ^ b
    if kind == 2:
        return bin((x | (x >> 1)) & 0x5555555555555555).count("1")
    return bin((x | (x >> 1) | (x >> 2)) & 0x9249249249249249).count("1")


def mix64(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def block_range(G, P, b):
    """Positions [lo, hi) of block b of P."""
    return G * b // P, G * (b + 1) // P


def block_mask(kind, G, P, b):
    lo, hi = block_range(G, P, b)
    lo, hi = lo * kind, min(64, hi * kind)
    return (((1 << (hi - lo)) - 1) << lo) & M64


def auto_code_bits(kind, whitelist, max_d):
    """The code_bits barcode.nearest_whitelist hands to the plan for this whitelist."""
    top = int(np.bitwise_or.reduce(np.asarray(whitelist, dtype=np.uint64))).bit_length()
    return min(64, max(top, kind * (max_d + 1)))


def dup_flags(whitelist):
    seen = {}
    for w in whitelist:
        seen[w] = seen.get(w, 0) + 1
    return [seen[w] > 1 for w in whitelist]


def oa_layout(kind, code_bits, max_d, nw, wrong=None):
    """dict(P, keys, keymasks, slots, groups, index_bytes), or None where the plan cannot take
    open addressing (more blocks than positions, or more than 6 keys)."""
    G = positions(kind, code_bits)
    P = 1 if max_d == 0 else max_d + 2
    keys = [(0, 0)] if max_d == 0 else [(a, b) for a in range(P) for b in range(a + 1, P)]
    if P > G or len(keys) > MAX_KEYS:
        return None
    bmask = [block_mask(kind, G, P, b) for b in range(P)]
    if wrong == "drop_last_block" and P > 1:
        keys = [(a, b) for a, b in keys if b != P - 1]
    slots = GROUP
    while slots < 2 * nw:
        slots *= 2
    return {"kind": kind, "G": G, "P": P, "keys": keys, "keymasks": [bmask[a] | bmask[b] for a, b in keys],
            "slots": slots, "groups": slots // GROUP, "index_bytes": len(keys) * slots * 16}


def oa_build(layout, whitelist):
    """One slot list per key: None or (code, index, dup), inserted in index order."""
    wl = [int(w) for w in whitelist]
    dup = dup_flags(wl)
    n, gmask = layout["slots"], layout["groups"] - 1
    tables = []
    for km in layout["keymasks"]:
        slots = [None] * n
        for j, w in enumerate(wl):
            s = (mix64(w & km) & gmask) * GROUP
            while slots[s] is not None:
                s = (s + 1) & (n - 1)
            slots[s] = (w, j, dup[j])
        tables.append(slots)
    return tables


def oa_probe(layout, tables, t, q):
    """The probe sequence of q in table t: (groups visited in order, entries visited)."""
    gmask = layout["groups"] - 1
    g = mix64(q & layout["keymasks"][t]) & gmask
    groups, seen = [], []
    while True:
        groups.append(g)
        for e in tables[t][g * GROUP:(g + 1) * GROUP]:
            if e is None:
                return groups, seen
            seen.append(e)
        g = (g + 1) & gmask


def oa_query(layout, tables, max_d, q, wrong=None):
    """(index, dist) of one query as oa_query_kernel walks the tables."""
    kind, gmask, ngroups = layout["kind"], layout["groups"] - 1, layout["groups"]
    best = [max_d + 1, -1, False]  # distance, index, tie

    def visit(e):
        d = dist(kind, q, e[0])
        if d <= best[0] and d <= max_d:
            if d < best[0]:
                best[0], best[1], best[2] = d, e[1], False
            elif e[1] != best[1] and wrong != "no_tie":
                best[2] = True

    if tables:  # the shortcut: a unique exact hit in table 0's first group
        g0 = mix64(q & layout["keymasks"][0]) & gmask
        hit = None
        for e in tables[0][g0 * GROUP:(g0 + 1) * GROUP]:
            if e is not None and e[0] == q and (not e[2] or wrong == "shortcut_ignores_dup"):
                hit = e
        if hit is not None:
            return hit[1], 0
    for t, slots in enumerate(tables):
        g = mix64(q & layout["keymasks"][t]) & gmask
        first = True
        while True:
            is_open = False
            for e in slots[g * GROUP:(g + 1) * GROUP]:
                if e is None:
                    is_open = True
                    break
                visit(e)
            if is_open or (first and wrong == "first_group_only"):
                break
            first = False
            if wrong == "no_wrap" and g + 1 == ngroups:
                break
            g = (g + 1) & gmask
    if best[1] < 0:
        return -1, 255
    return (-2 if best[2] else best[1]), best[0]


def _bucket(part, code):
    return ((((code & part["mask"]) >> part["lo_bit"]) * part["mul"]) & M64) >> part["shift"]


def _csr_provisional(kind, code_bits, max_d, nw):
    """(lg0, parts) of the provisional table: 2**lg0 ~ nw/2 buckets in every part."""
    G = positions(kind, code_bits)
    P = max_d + 1
    assert P <= MAX_PARTS and max_d < G
    lg0 = 0
    while lg0 < 28 and (1 << lg0) * 2 < nw:
        lg0 += 1
    parts = []
    for k in range(P):
        lo, hi = block_range(G, P, k)
        lo_bit = lo * kind
        nbits = min(64, hi * kind) - lo_bit
        parts.append({"mask": (((1 << nbits) - 1) << lo_bit) & M64, "lo_bit": lo_bit,
                      "mul": 0 if lg0 == 0 else GOLDEN, "shift": 63 if lg0 == 0 else 64 - lg0, "buckets": 1 << lg0})
    return lg0, parts


def csr_occupied(kind, code_bits, max_d, whitelist):
    """Per part the occupied buckets of the provisional table, which the build counts on the device
    (~ the part's distinct block values); zeros where the provisional table is one bucket and
    nothing is counted."""
    wl = [int(w) for w in whitelist]
    lg0, parts = _csr_provisional(kind, code_bits, max_d, len(wl))
    if not wl or lg0 == 0:
        return [0] * len(parts)
    return [len({_bucket(part, w) for w in wl}) for part in parts]


def csr_layout(kind, code_bits, max_d, nw, load, whitelist, wrong=None):
    """dict(parts: [mask, lo_bit, mul, shift, buckets], index_bytes) of the CSR plan; the bucket of
    a code in part k is csr_bucket(layout, k, code)."""
    wl = [int(w) for w in whitelist]
    assert len(wl) == nw
    G = positions(kind, code_bits)
    P = max_d + 1
    lg0, parts = _csr_provisional(kind, code_bits, max_d, nw)
    if nw and lg0 > 0:
        for part, occupied in zip(parts, csr_occupied(kind, code_bits, max_d, wl)):
            lg = 0
            while lg < lg0 and (1 << lg) < max(1, load) * max(1, occupied):
                lg += 1
            part.update(mul=0 if lg == 0 else GOLDEN, shift=63 if lg == 0 else 64 - lg, buckets=1 << lg)
    index_bytes = sum((p["buckets"] + 1) * 4 + nw * 12 for p in parts)
    if wrong == "drop_last_block" and P > 1:
        parts = parts[:-1]
    return {"kind": kind, "G": G, "P": P, "parts": parts, "index_bytes": index_bytes}


def csr_bucket(layout, k, code):
    return _bucket(layout["parts"][k], int(code))


def csr_build(layout, whitelist):
    """Per part: {bucket: [(code, index, dup), ...]}."""
    wl = [int(w) for w in whitelist]
    dup = dup_flags(wl)
    tables = []
    for part in layout["parts"]:
        b = {}
        for j, w in enumerate(wl):
            b.setdefault(_bucket(part, w), []).append((w, j, dup[j]))
        tables.append(b)
    return tables


def csr_query(layout, tables, max_d, q, wrong=None):
    """(index, dist) of one query as nearest_query_kernel scans its buckets."""
    kind = layout["kind"]
    best_d, best_j, tie, exact_unique = max_d + 1, -1, False, False
    if wrong == "no_distance_check":
        best_d = 1 << 30
    for part, buckets in zip(layout["parts"], tables):
        if exact_unique:
            break
        for w, j, dup in buckets.get(_bucket(part, q), ()):
            d = dist(kind, q, w)
            if d <= best_d and (d <= max_d or wrong == "no_distance_check"):
                if d < best_d:
                    best_d, best_j, tie = d, j, False
                    exact_unique = d == 0 and not dup
                elif j != best_j and wrong != "no_tie":
                    tie = True
    if best_j < 0:
        return -1, 255
    return (-2 if tie else best_j), min(best_d, 255)


def mirror_nearest(scheme, kind, code_bits, max_d, whitelist, queries, load=4, wrong=None):
    """(index list, dist list) of every query through the mirror of one layout, or None where the
    plan cannot take it."""
    wl = [int(w) for w in whitelist]
    if scheme == "oa":
        lay = oa_layout(kind, code_bits, max_d, len(wl), wrong=wrong)
        if lay is None:
            return None
        tables = oa_build(lay, wl)
        res = [oa_query(lay, tables, max_d, int(q), wrong=wrong) for q in queries]
    else:
        lay = csr_layout(kind, code_bits, max_d, len(wl), load, wl, wrong=wrong)
        tables = csr_build(lay, wl)
        res = [csr_query(lay, tables, max_d, int(q), wrong=wrong) for q in queries]
    return [r[0] for r in res], [r[1] for r in res]


def expected_scheme(forced, kind, code_bits, max_d, nw):
    """The scheme a plan reports when `forced` is 'oa' or 'csr'."""
    if forced == "oa" and oa_layout(kind, code_bits, max_d, nw) is not None:
        return "oa"
    return "csr"


def halves_packing(nw):
    """(pbits, ndw) of a half-key plan's permutation: 2 nw whitelist indices at pbits =
    max(1, ceil(log2 nw)) bits each, in dwords, and two more for the last entry's 8-byte load."""
    pbits = 1
    while pbits < 32 and (1 << pbits) < nw:
        pbits += 1
    return pbits, (2 * max(nw, 1) * pbits + 31) // 32 + 2


def halves_index_bytes(kind, code_bits, nw):
    """The index_bytes sct_nearest_plan_info reports for a half-key plan: the offsets of both tables
    (4**GA + 1 and 4**GB + 1 words; A the high ceil(G / 2) positions), nw uint16 entries in each, and
    the packed permutation in whole dwords, without its padding."""
    G = positions(kind, code_bits)
    GB = G // 2
    GA = G - GB
    pbits, _ = halves_packing(nw)
    return (4 ** GA + 4 ** GB + 2) * 4 + nw * 4 + (2 * nw * pbits + 31) // 32 * 4


# ---------------------------------------------------------------- part 2: the builders
def valid_digits(kind, code_bits, pos):
    """The A/C/G/T digit values that fit position `pos` of a code of code_bits bits (the top
    position of a width that is no multiple of `kind` holds fewer bits)."""
    room = min(kind, code_bits - kind * pos)
    return [v for v in ((0, 1, 2, 3) if kind == 2 else (1, 2, 3, 4)) if v < (1 << room)]


def set_digit(kind, code, pos, v):
    sh = kind * pos
    return ((code & ~(((1 << kind) - 1) << sh)) | (v << sh)) & M64


def get_digit(kind, code, pos):
    return (code >> (kind * pos)) & ((1 << kind) - 1)


def _random_code(rng, kind, code_bits, G):
    c = 0
    for p in range(G):
        vd = valid_digits(kind, code_bits, p)
        c |= vd[int(rng.integers(len(vd)))] << (kind * p)
    return c


def _substitute(rng, kind, code_bits, code, pos):
    """`code` with another A/C/G/T digit at `pos` (unchanged where the position holds one value)."""
    vd = [v for v in valid_digits(kind, code_bits, pos) if v != get_digit(kind, code, pos)]
    return set_digit(kind, code, pos, vd[int(rng.integers(len(vd)))]) if vd else code


def _distinct_codes(rng, kind, code_bits, G, n, taken=()):
    out, seen = [], set(taken)
    while len(out) < n:
        c = _random_code(rng, kind, code_bits, G)
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def _u64(values):
    return np.array(values, dtype=np.uint64)


def oa_chain_case(kind, L, max_d, nw, chain, dup=False, seed=0):
    """A whitelist of nw codes of L bases in which `chain` codes share the first pair key (blocks 0
    and 1; every block but the last, which tells them apart), the shared value searched until
    the key's first group is the last of the table: the chain fills it and runs on into group 0.
    max_d = 0 has one key, the whole code: the chain is `chain` copies of one code.  `dup`: the
    last chain code is a copy of the first (chain >= 2).  Queries: every code, every code with one
    base substituted at each position, and every code with one base substituted in each block past
    the first two (max_d away, found through the first pair key alone)."""
    code_bits = kind * L
    lay = oa_layout(kind, code_bits, max_d, nw)
    assert lay is not None and 1 <= chain <= nw
    rng = np.random.default_rng([seed, kind, L, max_d, nw, chain])
    G, P, last_group = L, lay["P"], lay["groups"] - 1
    trials = 0
    while True:  # seeded search for a shared value whose group is the table's last
        trials += 1
        shared = _random_code(rng, kind, code_bits, G)
        if mix64(shared & lay["keymasks"][0]) & last_group == last_group:
            break
    if max_d == 0:
        chain_codes = [shared] * chain
    else:
        lo, hi = block_range(G, P, P - 1)
        assert 4 ** (hi - lo) >= chain
        tail_mask = block_mask(kind, G, P, P - 1)
        seen, chain_codes = set(), []
        while len(chain_codes) < chain:  # distinct in the last block
            t = _random_code(rng, kind, code_bits, G) & tail_mask
            if t not in seen:
                seen.add(t)
                chain_codes.append((shared & ~tail_mask) | t)
        if dup and chain >= 2:
            chain_codes[-1] = chain_codes[0]
    others = _distinct_codes(rng, kind, code_bits, G, nw - chain, chain_codes)
    order = rng.permutation(nw)
    wl = [0] * nw
    for src, dst in enumerate(order):
        wl[int(dst)] = chain_codes[src] if src < chain else others[src - chain]
    chain_idx = sorted(int(d) for d in order[:chain])
    queries = list(wl)
    for w in wl:
        for p in range(G):
            queries.append(_substitute(rng, kind, code_bits, w, p))
        if max_d >= 1:  # one base in every block past the first two: only the first pair key is left
            c = w
            for b in range(2, P):
                b_lo, b_hi = block_range(G, P, b)
                c = _substitute(rng, kind, code_bits, c, int(rng.integers(b_lo, b_hi)))
            queries.append(c)
    info = {"layout": lay, "code_bits": code_bits, "chain_idx": chain_idx, "start_group": last_group,
            "trials": trials, "dup": bool(dup and chain >= 2 and max_d > 0) or (max_d == 0 and chain >= 2)}
    return _u64(wl), _u64(queries), info


OA_CHAINS = ((1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (9, 9), (13, 13), (3000, 700))
CSR_HEAVY_NW = (1, 2, 3, 4, 5, 8, 9, 16, 17)


def csr_heavy_case(kind, L, max_d, nw, block, seed=0):
    """nw distinct codes of L bases whose block `block` (of max_d + 1) is one constant: in that
    part one bucket holds the whole whitelist and every other is empty.  Queries: every code; every
    code with one base substituted at each position; every code with one base substituted in each
    other block (max_d away, found only through the heavy bucket); every code with max_d + 1 bases substituted
    outside the constant block where there is room (they meet the heavy bucket and mostly match
    nothing); random codes carrying the constant block.  info: per load 1 and 4 the mirror's
    layout, the heavy bucket's size and whether some bucket of another part holds two different
    block values."""
    code_bits = kind * L
    G, P = L, max_d + 1
    assert 0 <= block < P and max_d < G
    rng = np.random.default_rng([seed, kind, L, max_d, nw, block])
    const = _random_code(rng, kind, code_bits, G)
    cmask = block_mask(kind, G, P, block)
    lo, hi = block_range(G, P, block)
    free = [p for p in range(G) if not lo <= p < hi]
    wl, seen = [], set()
    if not free:  # max_d = 0: the block is the whole code, the whitelist nw copies of it
        wl = [const & cmask] * nw
    assert not free or 4 ** len(free) >= 2 * nw
    while len(wl) < nw:
        c = (_random_code(rng, kind, code_bits, G) & ~cmask) | (const & cmask)
        if c not in seen:
            seen.add(c)
            wl.append(c)
    queries = list(wl)
    for w in wl:
        for p in range(G):
            queries.append(_substitute(rng, kind, code_bits, w, p))
        if max_d >= 1:  # one base in every other block: max_d away, met only in the heavy bucket
            c = w
            for k in range(P):
                b_lo, b_hi = block_range(G, P, k)
                if k != block:
                    c = _substitute(rng, kind, code_bits, c, int(rng.integers(b_lo, b_hi)))
            queries.append(c)
        if len(free) >= max_d + 1:
            c = w
            for p in rng.permutation(len(free))[:max_d + 1]:
                c = _substitute(rng, kind, code_bits, c, free[int(p)])
            queries.append(c)
    for _ in range(8):
        queries.append((_random_code(rng, kind, code_bits, G) & ~cmask) | (const & cmask))
    info = {"code_bits": code_bits, "block": block}
    for load in (1, 4):
        lay = csr_layout(kind, code_bits, max_d, nw, load, wl)
        tables = csr_build(lay, wl)
        shared = False
        for k, part in enumerate(lay["parts"]):
            if k == block:
                continue
            for entries in tables[k].values():
                if len({e[0] & part["mask"] for e in entries}) > 1:
                    shared = True
        info[load] = {"layout": lay, "heavy": len(tables[block].get(csr_bucket(lay, block, const), ())),
                      "heavy_part_buckets": len(tables[block]), "shared": shared}
    return _u64(wl), _u64(queries), info


def valid_space(kind, code_bits):
    n = 1
    for p in range(positions(kind, code_bits)):
        n *= len(valid_digits(kind, code_bits, p))
    return n


def width_case(kind, code_bits, nw, nq, seed=0):
    """A whitelist of min(nw, space) distinct A/C/G/T codes below 2**code_bits, one of them with
    bit code_bits - 1 set (barcode.nearest_whitelist then derives this code_bits), followed by its
    first 3 codes again (ties at distance 0).  Queries in six classes: exact; 1..3 substituted
    bases; for kind 3, an N (6) or an invalid triplet 0, 5, 7; one bit set above code_bits (at
    most bit 63); uniformly random, below 2**code_bits and over all 64 bits.

    Where the space allows (4**G >= 4 * nw) four random codes z0..z3 are kept clear: no whitelist
    code lies within 3 of z0, and within m of z_m (m = 1, 2, 3) lies exactly one, z_m with m bases
    substituted.  The z's are queries, so at every max_d <= 3 the set holds a query answered
    uniquely at exactly max_d (z_max_d) and one answered by nothing (z0); a dense whitelist (300 codes
    among 4**6) leaves neither to chance.  info['classes'] names each query's class."""
    G = positions(kind, code_bits)
    rng = np.random.default_rng([seed, kind, code_bits, nw, nq])
    space = valid_space(kind, code_bits)
    n = min(nw, space)
    holes, specials = [], []
    full = [p for p in range(G) if len(valid_digits(kind, code_bits, p)) == 4]
    if 4 ** G >= 4 * nw and len(full) >= 6:
        for _ in range(10000):
            holes = _distinct_codes(rng, kind, code_bits, G, 4)
            specials = []
            for m in (1, 2, 3):
                s = holes[m]
                for p in rng.permutation(len(full))[:m]:
                    s = _substitute(rng, kind, code_bits, s, full[int(p)])
                specials.append(s)
            ok = len(set(specials)) == 3
            for i, s in enumerate(specials):
                ok = ok and dist(kind, s, holes[0]) > 3
                ok = ok and all(dist(kind, s, holes[m]) > m for m in (1, 2, 3) if m != i + 1)
            if ok:
                break
        else:
            raise AssertionError("no clear codes found")

    def clear(c):
        if not holes:
            return True
        return dist(kind, c, holes[0]) > 3 and all(dist(kind, c, holes[m]) > m for m in (1, 2, 3))

    pool, seen = [], set(specials)
    if space <= 1 << 16:  # a small space: enumerate it in random order
        cand = [0]
        for p in range(G):
            cand = [c | (v << (kind * p)) for c in cand for v in valid_digits(kind, code_bits, p)]
        for i in rng.permutation(len(cand)):
            if len(pool) < n - len(specials) and cand[int(i)] not in seen and clear(cand[int(i)]):
                pool.append(cand[int(i)])
    else:
        while len(pool) < n - len(specials):
            c = _random_code(rng, kind, code_bits, G)
            if c not in seen and clear(c):
                seen.add(c)
                pool.append(c)
    if not any(c >> (code_bits - 1) for c in pool + specials):  # the top bit, for auto_code_bits
        top = [v for v in valid_digits(kind, code_bits, G - 1) if (v << (kind * (G - 1))) >> (code_bits - 1)]
        for i, c in enumerate(pool):
            c2 = set_digit(kind, c, G - 1, top[0])
            if c2 not in pool and c2 not in specials and clear(c2):
                pool[i] = c2
                break
    wl = pool[:3] + specials + pool[3:]
    wl = wl + wl[:3]
    queries, classes = list(holes) + wl[:3], ["hole"] * len(holes) + ["exact"] * 3  # (the duplicated codes: ties)
    shares = (("exact", 0.25), ("sub", 0.30), ("odd", 0.15 if kind == 3 else 0.0), ("high", 0.10), ("random", 1.0))
    while len(queries) < nq:
        u, name = rng.random(), None
        for name, share in shares:
            if u < share:
                break
            u -= share
        q = wl[int(rng.integers(len(wl)))]
        if name == "sub":
            for p in rng.permutation(G)[:int(rng.integers(1, 4))]:
                q = _substitute(rng, kind, code_bits, q, int(p))
        elif name == "odd":
            q = set_digit(3, q, int(rng.integers(G)), (6, 6, 0, 5, 7)[int(rng.integers(5))])
            if rng.random() < 0.5:
                q = _substitute(rng, kind, code_bits, q, int(rng.integers(G)))
        elif name == "high":
            if code_bits < 64:
                q |= 1 << int(rng.integers(code_bits, 64))
            if rng.random() < 0.5:
                q = _substitute(rng, kind, code_bits, q, int(rng.integers(G)))
        elif name == "random":
            q = int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(2))
            if rng.random() < 0.5:
                q &= (1 << code_bits) - 1
        queries.append(q)
        classes.append(name)
    queries, classes = queries[:nq], classes[:nq]
    return _u64(wl), _u64(queries), {"code_bits": code_bits, "G": G, "holes": len(holes), "classes": classes}


def odd_whitelist_case(L, seed=0):
    """ThreeBit whitelists that are not A/C/G/T: 200 random codes of L bases, five of them changed
    to hold an N (6), a 0 in the middle, a 5, a 7, and a code one base short (top triplet 0).
    Queries: every code; every changed code with one base substituted at each other position; every
    plain code with the same odd triplets at the changed codes' positions and at other positions
    (N against N is distance 0 under the XOR rule); one substitution of every code."""
    kind, code_bits, G = 3, 3 * L, L
    rng = np.random.default_rng([seed, L])
    wl = _distinct_codes(rng, kind, code_bits, G, 200)
    where = [int(i) for i in rng.permutation(len(wl))[:5]]
    odd = [(6, int(rng.integers(G))), (0, G // 2), (5, int(rng.integers(G))), (7, int(rng.integers(G))), (0, G - 1)]
    for i, (v, p) in zip(where, odd):
        wl[i] = set_digit(kind, wl[i], p, v)
    queries = list(wl)
    for i, (v, p) in zip(where, odd):
        for p2 in range(G):
            if p2 != p:
                queries.append(_substitute(rng, kind, code_bits, wl[i], p2))
    for w in wl:
        queries.append(_substitute(rng, kind, code_bits, w, int(rng.integers(G))))
        v, p = odd[int(rng.integers(len(odd)))]
        queries.append(set_digit(kind, w, p, v))  # the same triplet at the same position
        queries.append(set_digit(kind, w, int(rng.integers(G)), v))  # and at another
    for i in where:  # an N where the changed code has its odd triplet, and beside it
        for v, p in odd:
            queries.append(set_digit(kind, wl[i], p, 6))
            queries.append(set_digit(kind, set_digit(kind, wl[i], p, 6), (p + 1) % G, 6))
    return _u64(wl), _u64(queries), {"code_bits": code_bits, "odd_idx": where, "odd": odd}
