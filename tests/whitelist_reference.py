"""A plain reading of whitelist ingest, and inputs that put one feature on one seam of the device
code (sctools_amd/csrc/lines.hip, tile_prefix.h).

Part 1, the reference: the lines of a file as barcode.py:95-97 reads them -- a binary file iterated
line by line (io.BytesIO(data).readlines()), `line[:-1]` of each -- with every line's start and
chopped length, and each chopped line's code limbs, GC count and flags from
tests/encode_reference.py (encode_var for one limb, encode for more).  A line too long for `words`
limbs carries flag 4, zero limbs and zero gc; gc saturates at 255.  Nothing of the device layout is
known to this part.

Part 2, the seam cases: deterministic (data, desc, claims) with one feature -- a '\\n', an empty
line, a split line, a long line, the file's end, a capacity -- at byte S + d of a five-tile buffer,
and fixed-stride files whose lines pass every tile seam.  Every claim is checked on the CPU
(tests/test_whitelist_reference_host.py) before a GPU test relies on it.

Part 3, the coarse pieces: more than 1,024 tiles of 20,000-byte lines, one line longer than a
block of 32 tiles, and clusters of short lines around the tiles where a block of 32 or of 1,024
tiles ends.
"""

import io
from collections import namedtuple

import numpy as np

import encode_reference as E

# ---------------------------------------------------------------- part 1: the reference
Lines = namedtuple("Lines", "n maxlen starts lens")
Enc = namedtuple("Enc", "codes gc flags")
F_LONG = 4  # a line too long for the limbs asked for


def read_lines(data):
    """Lines(n, the longest chopped length, start int64[n], chopped length int32[n])."""
    raw = io.BytesIO(data).readlines()
    full = np.fromiter((len(x) for x in raw), np.int64, len(raw))
    starts = np.zeros(len(raw), np.int64)
    starts[1:] = np.cumsum(full)[:-1]
    lens = np.fromiter((len(x[:-1]) for x in raw), np.int64, len(raw)).astype(np.int32)
    return Lines(len(raw), int(lens.max(initial=0)), starts, lens)


def encode_lines(data, lines, kind, words):
    """Enc(codes (n, words) uint64 little-endian limbs, gc uint8[n], flags uint8[n]) of the chopped
    lines."""
    buf = np.frombuffer(data, np.uint8)
    lens = lines.lens.astype(np.int64)
    codes = np.zeros((lines.n, words), np.uint64)
    gc = np.zeros(lines.n, np.uint8)
    flags = np.zeros(lines.n, np.uint8)
    flags[kind * lens > 64 * words] = F_LONG
    one = np.flatnonzero(kind * lens <= 64)
    codes[one, 0], gc[one], flags[one] = E.encode_var(kind, buf, lines.starts[one], lens[one])
    more = (kind * lens > 64) & (kind * lens <= 64 * words)
    for L in np.unique(lens[more]).tolist():
        rows = np.flatnonzero(more & (lens == L))
        recs = buf[lines.starts[rows][:, None] + np.arange(L)[None, :]]
        codes[rows], gc[rows], flags[rows] = E.encode(kind, recs, words)
    return Enc(codes, gc, flags)


# ---------------------------------------------------------------- part 2: seam cases
# The seams of the device code: a lane's 16 bytes, a wave's 1 KiB of a sub-tile, the 4 KiB sub-tile,
# the 16 KiB tile and its multiples (a workgroup's range of 1, 2 or 3 tiles starts or ends there).
LANE, WAVE, SUB, TILE = 16, 1024, 4096, 16384
SEAMS = (LANE, WAVE, SUB, TILE, 2 * TILE, 3 * TILE)
PHASES = (-2, -1, 0, 1, 2)
NBUF = 5 * TILE
LONG = 40_000
LINES_TILE = 4096  # sct_lines' own tile

# claims: ("byte", offset, value); ("byte_not", offset, value); ("n", size); ("tiles", count of
# 16 KiB tiles); ("no_lf_tile", k) tile k holds no '\n'; ("line", start, length) the reference has
# that line; ("clean_line", start, length) and it holds A/C/G/T/acgt only (flags 0);
# ("flag_line", start, length, TwoBit flags); ("cap", capacity) the case runs with it;
# ("stride", S) every line is S bytes with its '\n' (the last one may lack it); ("straddle", offset)
# a line has bytes before offset and bytes (its '\\n' at the least) at or past it
Case = namedtuple("Case", "data desc claims")

_rng = np.random.default_rng(20240607)
UPAT = np.frombuffer(b"ACGT", np.uint8)[_rng.integers(0, 4, 1 << 16)].tobytes()
MPAT = np.frombuffer(b"ACGTacgt", np.uint8)[_rng.integers(0, 8, 1 << 12)].tobytes()
del _rng


def upper(i, L):
    """Line i of L upper-case bases."""
    o = (37 * i) % 1009
    assert o + L <= len(UPAT)
    return UPAT[o:o + L]


def mixed(i, L):
    o = (53 * i) % 997
    return MPAT[o:o + L]


def _fill_stream(nbytes):
    """Whole lines of cycling length 0 .. 40, every third one with lower-case bases."""
    out, ends, size, i = [], [], 0, 0
    while size < nbytes:
        L = i % 41
        out.append((mixed(i, L) if i % 3 == 2 else upper(i, L)) + b"\n")
        size += L + 1
        ends.append(size)
        i += 1
    return b"".join(out), np.array(ends, np.int64)


_FILL, _FILL_ENDS = _fill_stream(NBUF + 64)


def filler(P):
    """Exactly P bytes of whole clean '\\n'-ended lines (the last one cut to fit)."""
    assert 0 <= P <= NBUF
    k = int(np.searchsorted(_FILL_ENDS, P, side="right"))
    done = int(_FILL_ENDS[k - 1]) if k else 0
    out = _FILL[:done]
    if P > done:
        out += upper(k, P - done - 1) + b"\n"
    return out


def _case(desc, head, blob, claims, total=NBUF):
    """`head` bytes of filler, the blob, filler up to `total`."""
    body = filler(head) + blob
    data = body + filler(total - len(body))
    return Case(data, desc, list(claims) + [("n", total), ("tiles", -(-total // TILE))])


def _short(S):
    return 8 if S == LANE else 20


def family_lf():
    """A clean line's '\\n' at S + d."""
    out = []
    for S in SEAMS:
        L = _short(S)
        for d in PHASES:
            at = S + d
            out.append(_case("lf at S=%d d=%+d" % (S, d), at - L, upper(at, L) + b"\n",
                             [("byte", at, 10), ("clean_line", at - L, L)]))
    return out


def family_empty():
    """Two consecutive '\\n' at S + d - 1 and S + d: an empty line that starts at S + d."""
    out = []
    for S in SEAMS:
        L = 6 if S == LANE else 20
        for d in PHASES:
            at = S + d
            out.append(_case("empty line at S=%d d=%+d" % (S, d), at - 1 - L, upper(at, L) + b"\n\n",
                             [("byte", at - 1, 10), ("byte", at, 10), ("clean_line", at - 1 - L, L),
                              ("clean_line", at, 0)]))
    return out


def family_split():
    """A clean line of 32 bases with k bytes before the seam and 32 - k after it, k = 1 .. 31."""
    out = []
    for S in SEAMS:
        for k in range(1, 32):
            if k > S:
                continue
            out.append(_case("32 bases split %d | %d at S=%d" % (k, 32 - k, S), S - k, upper(S + k, 32) + b"\n",
                             [("byte", S - k + 32, 10), ("clean_line", S - k, 32), ("straddle", S)]))
    return out


def family_long():
    """A line of 40,000 bytes that starts at S + d (ends there for the last seam): the tiles under
    it hold no line end."""
    out = []
    for S in SEAMS:
        for d in PHASES:
            at = S + d
            start = at if at + LONG + 1 <= NBUF else at - LONG
            inner = range(-(-start // TILE), (start + LONG) // TILE)
            claims = [("line", start, LONG), ("byte", start + LONG, 10)] + [("no_lf_tile", k) for k in inner]
            assert len(claims) > 2
            if start:
                claims.append(("byte", start - 1, 10))
            out.append(_case("line of %d bytes %s S=%d d=%+d" % (LONG, "from" if start == at else "up to", S, d),
                             start, upper(at, LONG) + b"\n", claims))
    return out


def family_end():
    """The file ends at S + d, with a final '\\n' and without one (the last base is chopped)."""
    out = []
    for S in SEAMS + (NBUF,):
        L = _short(S)
        for d in PHASES:
            N = S + d
            for fin in (True, False):
                last = upper(N, L) + (b"\n" if fin else upper(N + 1, 1))
                claims = [("byte" if fin else "byte_not", N - 1, 10), ("clean_line", N - L - 1, L)]
                out.append(_case("file end at S=%d d=%+d %s a final lf" % (S, d, "with" if fin else "without"),
                                 N - L - 1, last, claims, total=N))
    return out


def family_cap():
    """The capacity is the number g of the line whose '\\n' is at S + d, and g - 1, g + 1."""
    out = []
    for c in family_lf():
        at = c.claims[0][1]
        g = c.data[:at].count(b"\n")
        for delta in (-1, 0, 1):
            assert g + delta >= 0
            out.append(Case(c.data, "capacity %d, line %d: %s" % (g + delta, g, c.desc), c.claims + [("cap", g + delta)]))
    return out


FIXED_STRIDES = (17, 13, 22, 33)
FIXED_BYTES = 5 * TILE + 5000


def fixed_case(S, fin=True, lut=True):
    """Lines of S - 1 upper-case bases over 5 tiles and a part of a sixth; with `lut` the line over
    the first tile seam is lower-case and the one over the second holds an N."""
    n = FIXED_BYTES // S
    lines = [upper(i, S - 1) for i in range(n)]
    g1, g2 = TILE // S, 2 * TILE // S
    claims = [("stride", S)] + [("straddle", k * TILE) for k in range(1, 6)]
    if lut:
        lines[g1] = lines[g1].lower()
        lines[g2] = lines[g2][:S // 2] + b"N" + lines[g2][S // 2 + 1:]
        claims += [("flag_line", g1 * S, S - 1, 0), ("byte", g1 * S, ord(upper(g1, 1).lower())),
                   ("flag_line", g2 * S, S - 1, 1)]
    data = b"\n".join(lines) + b"\n"
    if not fin:  # the last line is then S - 1 bytes, its last base chopped
        data = data[:-1]
        claims += [("byte_not", len(data) - 1, 10), ("clean_line", (n - 1) * S, S - 2)]
    claims += [("n", len(data)), ("tiles", 6)]
    return Case(data, "stride %d%s%s" % (S, "" if fin else ", no final lf", "" if lut else ", upper case only"), claims)


def family_fixed():
    out = [fixed_case(S, fin) for S in FIXED_STRIDES for fin in (True, False)]
    return out + [fixed_case(13, lut=False)]


def family_gc():
    """Lines of 300 G / C bases (gc saturates at 255) and of 254 .. 257."""
    lines = [b"G" * 300, b"GC" * 150, b"G" * 254 + b"A" * 46, b"C" * 255, b"G" * 256, b"g" * 257, b"A" * 300]
    blob = b"\n".join(lines) + b"\n"
    claims = [("line", TILE - 700 + sum(len(x) + 1 for x in lines[:k]), len(lines[k])) for k in range(len(lines))]
    return [_case("lines of up to 300 G/C over the first tile seam", TILE - 700, blob, claims, total=2 * TILE)]


FAMILIES = {"lf": family_lf, "empty": family_empty, "split": family_split, "long": family_long,
            "end": family_end, "cap": family_cap, "fixed": family_fixed}
GC_FAMILY = "gc"  # ten limbs: run on its own

_cache = {}


def cases(family):
    if family not in _cache:
        _cache[family] = family_gc() if family == GC_FAMILY else FAMILIES[family]()
    return _cache[family]


def claim(case, kind):
    return [c for c in case.claims if c[0] == kind]


def check_claims(case):
    data = case.data
    ref = read_lines(data)
    have = dict(zip(ref.starts.tolist(), ref.lens.tolist()))
    enc = None
    for c in case.claims:
        what = (case.desc, c)
        if c[0] == "byte":
            assert 0 <= c[1] < len(data) and data[c[1]] == c[2], what
        elif c[0] == "byte_not":
            assert 0 <= c[1] < len(data) and data[c[1]] != c[2], what
        elif c[0] == "n":
            assert len(data) == c[1], what
        elif c[0] == "tiles":
            assert -(-len(data) // TILE) == c[1], what
        elif c[0] == "no_lf_tile":
            assert len(data) >= (c[1] + 1) * TILE and b"\n" not in data[c[1] * TILE:(c[1] + 1) * TILE], what
        elif c[0] in ("line", "clean_line", "flag_line"):
            assert have.get(c[1]) == c[2], what
            if c[0] != "line":
                enc = enc or encode_lines(data, ref, 2, 2)
                g = int(np.searchsorted(ref.starts, c[1]))
                assert enc.flags[g] == (c[3] if c[0] == "flag_line" else 0), what
        elif c[0] == "cap":
            assert 0 <= c[1] <= ref.n, what
        elif c[0] == "stride":
            ends = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
            assert np.array_equal(ends, np.arange(ends.size) * c[1] + c[1] - 1), what
            assert len(data) in (ends.size * c[1], (ends.size + 1) * c[1] - 1), what
        else:
            assert c[0] == "straddle", what
            g = int(np.searchsorted(ref.starts, c[1], side="right")) - 1
            assert ref.starts[g] < c[1] <= ref.starts[g] + ref.lens[g], what


# ---------------------------------------------------------------- part 3: the coarse pieces
# The count pass sums its tiles' line ends over blocks of 32 and of 1,024 tiles; a tile's first line
# number and the last line end before it come from those sums (or from all the tiles before it).
COARSE_TILES = 1058
COARSE_LINE, COARSE_LONG = 20_000, 600 * 1024
COARSE_EMPTY_BLOCK = 2  # tiles 64 .. 95 lie under the long line


def coarse_clusters(ntiles):
    """The first tile of every cluster of three tiles of short lines."""
    at = [31, 255, 1023, ntiles - 3]
    assert all(a + 3 <= b for a, b in zip(at, at[1:])) and at[0] > 0
    return at


def coarse_piece(ntiles):
    """ntiles whole tiles: lines of 20,000 bytes, one of 600 KiB over a whole block of 32 tiles,
    three tiles of short clean lines around tiles 31 / 32 / 33, 255 / 256 / 257, 1,023 / 1,024 /
    1,025 and at the end."""
    N = ntiles * TILE
    buf = bytearray((UPAT * (N // len(UPAT) + 1))[:N])
    a = COARSE_EMPTY_BLOCK * 32 * TILE - 40_000  # the long line: [a, a + COARSE_LONG) and its '\n'
    for p in range(COARSE_LINE - 1, N, COARSE_LINE):
        if not a <= p < a + COARSE_LONG:
            buf[p] = 10
    buf[a - 1] = 10
    buf[a + COARSE_LONG] = 10
    for t in coarse_clusters(ntiles):
        buf[t * TILE:(t + 3) * TILE] = filler(3 * TILE)
    assert len(buf) == N
    return bytes(buf)


def lf_per_tile(data, tile=TILE):
    a = np.frombuffer(data, np.uint8)
    return np.bincount(np.flatnonzero(a == 10) // tile, minlength=-(-len(data) // tile))


def check_coarse(data, ntiles):
    """What a coarse piece promises, from its bytes."""
    assert len(data) == ntiles * TILE and data[-1] == 10
    per = lf_per_tile(data)
    blk = COARSE_EMPTY_BLOCK
    assert not per[32 * blk:32 * blk + 32].any() and per[:32 * blk].any()  # a whole block without a line end
    for t in coarse_clusters(ntiles):
        assert (per[t:t + 3] > 300).all(), (t, per[t:t + 3])
    rest = np.ones(ntiles, bool)
    for t in coarse_clusters(ntiles):
        rest[t - 1:t + 4] = False
    assert per[rest].max() <= 2 and (per[rest] == 0).sum() > ntiles // 8  # tiles without a line end throughout
    ref = read_lines(data)
    assert ref.maxlen == COARSE_LONG and (ref.lens == COARSE_LINE - 1).sum() > ntiles // 2
    return ref


EMPTY_LINES = 600_000  # more lines than sct_lines' length pass has threads (2,048 x 256)
