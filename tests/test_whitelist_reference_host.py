"""tests/whitelist_reference.py pinned on the CPU: every seam case's claims -- the byte at S + d,
the buffer size, the tile count, the tiles without a '\\n', the lines it says it holds -- the
reference against a real file read the way barcode.py:95-97 reads it, its codes against the
oracle's encoders, and the cap on what a device test may leave uncompared."""

import numpy as np
import pytest

import encode_reference as E
import whitelist_reference as W
from oracle import oracle as O

ALL = sorted(W.FAMILIES) + [W.GC_FAMILY]


@pytest.mark.parametrize("family", ALL)
def test_every_seam_case_holds_its_claims(family):
    cs = W.cases(family)
    assert cs and len({c.desc for c in cs}) == len(cs)  # descriptions name the cases
    for c in cs:
        assert W.claim(c, "n") and W.claim(c, "tiles")
        W.check_claims(c)
        assert len(c.data) <= W.NBUF + 5000 + 2
    assert W.cases(family) is cs  # built once, shared


def test_seam_families_cover_the_seams():
    """The phases the families promise, read back from the claims."""
    want = {S + d for S in W.SEAMS for d in W.PHASES}
    assert want == {c.claims[0][1] for c in W.cases("lf")}
    assert want == {c.claims[1][1] for c in W.cases("empty")}  # (the second '\n': the empty line's start)
    starts = {W.claim(c, "line")[0][1] for c in W.cases("long")}
    ends = {W.claim(c, "line")[0][1] + W.LONG for c in W.cases("long")}
    assert want == {x for x in starts | ends if x in want} and len(W.cases("long")) == len(want)
    for fin in ("byte", "byte_not"):  # the file's end with and without a final '\n'
        sizes = {c.claims[0][1] + 1 for c in W.cases("end") if c.claims[0][0] == fin}
        assert sizes == want | {W.NBUF + d for d in W.PHASES}
    split = {(W.claim(c, "straddle")[0][1], W.claim(c, "straddle")[0][1] - W.claim(c, "clean_line")[0][1])
             for c in W.cases("split")}
    assert split == {(S, k) for S in W.SEAMS for k in range(1, 32) if k <= S}
    # the capacities: the seam line's number, one below, one above
    by_data = {}
    for c in W.cases("cap"):
        by_data.setdefault(c.data, []).append(W.claim(c, "cap")[0][1])
    assert len(by_data) == len(want)
    for data, caps in by_data.items():
        at = next(c for c in W.cases("lf") if c.data == data).claims[0][1]
        g = int(np.searchsorted(W.read_lines(data).starts, at, side="right")) - 1  # the line that holds byte S + d
        assert caps == [g - 1, g, g + 1]
    # the five-tile buffer, except where the file's end is the feature
    for fam in ("lf", "empty", "split", "long", "cap"):
        assert all(len(c.data) == W.NBUF for c in W.cases(fam))
    # the long line leaves at least one whole tile without a line end, the last seam's two
    assert all(W.claim(c, "no_lf_tile") for c in W.cases("long"))
    assert max(len(W.claim(c, "no_lf_tile")) for c in W.cases("long")) == 2


def test_fixed_stride_files():
    cs = W.cases("fixed")
    assert [W.claim(c, "stride")[0][1] for c in cs] == [17, 17, 13, 13, 22, 22, 33, 33, 13]
    for c in cs:
        S = W.claim(c, "stride")[0][1]
        ref = W.read_lines(c.data)
        assert len(c.data) > 5 * W.TILE and ref.n == W.FIXED_BYTES // S
        fin = not W.claim(c, "byte_not")
        assert (len(c.data) % S == 0) == fin and ref.lens[:-1].tolist() == [S - 1] * (ref.n - 1)
        assert ref.lens[-1] == (S - 1 if fin else S - 2)
        assert len(W.claim(c, "straddle")) == 5
        enc = W.encode_lines(c.data, ref, 2, 2)
        lut = W.claim(c, "flag_line")
        if lut:  # one lower-case line (flags 0) and one with an N (flags 1), each over a tile seam
            assert [x[3] for x in lut] == [0, 1] and np.flatnonzero(enc.flags).size == 1
            assert c.data[lut[0][1]:lut[0][1] + S - 1].islower() and b"N" in c.data[lut[1][1]:lut[1][1] + S - 1]
            assert lut[0][1] < W.TILE < lut[0][1] + S and lut[1][1] < 2 * W.TILE < lut[1][1] + S
        else:
            assert not enc.flags.any() and c.data.isupper()


@pytest.mark.parametrize("family", ALL)
def test_reference_equals_a_file_read_line_by_line(family, tmp_path):
    """open(p, 'rb'), iterate, line[:-1]: barcode.py:95-97."""
    cs = W.cases(family)
    pick = cs if family in ("end", "fixed", "empty", W.GC_FAMILY) else cs[::7]
    p = tmp_path / "whitelist.txt"
    for c in pick:
        p.write_bytes(c.data)
        with open(p, "rb") as f:
            chopped = [line[:-1] for line in f]
        ref = W.read_lines(c.data)
        assert ref.n == len(chopped) and ref.maxlen == max(map(len, chopped), default=0), c.desc
        got = [c.data[s:s + n] for s, n in zip(ref.starts.tolist(), ref.lens.tolist())]
        assert got == chopped, c.desc


def test_reference_small_files():
    for data, want in ((b"", []), (b"A", [(0, 0)]), (b"\n", [(0, 0)]), (b"ACGT\nAC\n\nGGGGG\nT", [(0, 4), (5, 2), (8, 0), (9, 5), (15, 0)]),
                       (b"AC\r\nG", [(0, 3), (4, 0)])):
        ref = W.read_lines(data)
        assert list(zip(ref.starts.tolist(), ref.lens.tolist())) == want and ref.n == len(want)
        assert ref.maxlen == max([n for _, n in want], default=0)


@pytest.mark.parametrize("family", ALL)
def test_reference_codes_equal_the_oracle(family):
    """A sample of every case's lines through the oracle's own encoders: clean lines by value,
    every sampled line's flags by the oracle's maps."""
    seen = 0
    for c in W.cases(family)[::5]:
        ref = W.read_lines(c.data)
        for kind, words in ((2, 1), (3, 1), (2, 2)) if family != W.GC_FAMILY else ((2, 10),):
            enc = W.encode_lines(c.data, ref, kind, words)
            marks = [x[1] for x in c.claims if x[0] in ("line", "clean_line", "flag_line")]
            rows = sorted(set(range(0, ref.n, 53)) | {int(np.searchsorted(ref.starts, m)) for m in marks} | {ref.n - 1})
            for g in rows:
                s, n = int(ref.starts[g]), int(ref.lens[g])
                rec = c.data[s:s + n]
                if kind * n > 64 * words:
                    assert (enc.flags[g], enc.gc[g], E.ints(enc.codes[g:g + 1])[0]) == (W.F_LONG, 0, 0), (c.desc, g)
                    continue
                amb = kind == 2 and any(b in O._AMBIG for b in rec)
                bad = kind == 2 and any(b not in O._TWO and b not in O._AMBIG for b in rec)
                assert enc.flags[g] == (1 if amb else 0) | (2 if bad else 0), (c.desc, g)
                if amb or bad:
                    continue
                code = E.ints(enc.codes[g:g + 1])[0]
                if kind == 2:
                    assert code == O.two_bit_encode(rec) and enc.gc[g] == min(255, O.two_bit_gc(code, n)), (c.desc, g)
                else:
                    assert code == O.three_bit_encode(rec) and enc.gc[g] == min(255, O.three_bit_gc(code)), (c.desc, g)
                seen += 1
    assert seen > 20


def test_reference_long_lines_and_saturated_gc():
    (c,) = W.cases(W.GC_FAMILY)
    ref = W.read_lines(c.data)
    rows = [int(np.searchsorted(ref.starts, x[1])) for x in W.claim(c, "line")]
    enc = W.encode_lines(c.data, ref, 2, 10)
    assert enc.gc[rows].tolist() == [255, 255, 254, 255, 255, 255, 0] and not enc.flags.any()
    enc = W.encode_lines(c.data, ref, 2, 9)  # 576 bits: the lines of 300 bases do not fit
    assert enc.flags[rows].tolist() == [4, 4, 4, 0, 0, 0, 4] and enc.gc[rows].tolist() == [0, 0, 0, 255, 255, 255, 0]
    assert not enc.codes[rows][[0, 1, 2, 6]].any() and enc.codes[rows][[3, 4, 5]].any(axis=1).all()
    # (kind, words) of the device tests: the filler's lines of 33 .. 40 and 22 .. 40 bases are too long
    c = W.cases("lf")[7]
    ref = W.read_lines(c.data)
    for kind, words, fit in ((2, 1, 32), (3, 1, 21), (2, 2, 64)):
        enc = W.encode_lines(c.data, ref, kind, words)
        assert np.array_equal(enc.flags == 4, ref.lens > fit) and not enc.codes[ref.lens > fit].any()
        assert not enc.gc[ref.lens > fit].any() and (enc.flags == 4).any() == (fit < 40)


@pytest.mark.parametrize("family", ALL)
def test_skip_cap(family):
    """The device tests compare every limb of every line.  Should one ever leave a line's code
    uncompared, it may only be a line whose reference flags are not zero: here the lines a claim
    puts on a seam are clean, and lines with an ambiguous or invalid byte are at most 5 % of any
    case's lines (the reference alone decides both)."""
    for c in W.cases(family):
        ref = W.read_lines(c.data)
        enc = W.encode_lines(c.data, ref, 2, 10)
        assert np.count_nonzero(enc.flags & 3) <= 0.05 * ref.n, c.desc
        for _, start, n in W.claim(c, "clean_line"):
            g = int(np.searchsorted(ref.starts, start))
            assert (ref.starts[g], ref.lens[g], enc.flags[g]) == (start, n, 0), (c.desc, start)
            assert all(b in b"ACGTacgt" for b in c.data[start:start + n])
        if family in ("lf", "empty", "split", "end", "cap"):
            assert W.claim(c, "clean_line"), c.desc


@pytest.mark.parametrize("ntiles", (W.COARSE_TILES, 256 * 8 + 3, 304 * 8 + 3))
def test_coarse_pieces_hold_their_claims(ntiles):
    """Piece (a) and piece (b) for a device of 256 or 304 compute units: a whole block of 32 tiles
    without a line end, clusters of short lines around tiles 31-33, 255-257, 1,023-1,025 and in the
    last three tiles, lines of 20,000 bytes elsewhere; all of it clean."""
    data = W.coarse_piece(ntiles)
    ref = W.check_coarse(data, ntiles)
    assert ntiles > 1025 + 3 and W.coarse_clusters(ntiles) == [31, 255, 1023, ntiles - 3]
    enc = W.encode_lines(data, ref, 2, 1)
    assert not (enc.flags & 3).any() and (enc.flags == 4).sum() > ntiles // 2 and (enc.flags == 0).sum() > 4000
    # line ends on both sides of every block seam of the clusters
    a = np.frombuffer(data, np.uint8)
    for t in (32, 256, 1024):
        assert (a[t * W.TILE - 64:t * W.TILE] == 10).any() and (a[t * W.TILE:t * W.TILE + 64] == 10).any()


def test_empty_lines_buffer_passes_the_length_grid():
    assert W.EMPTY_LINES > 2048 * 256 and W.EMPTY_LINES // W.LINES_TILE > 100
