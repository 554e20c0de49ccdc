"""tests/fastq_reference.py pinned on the CPU: the reference against every case of
tests/golden/fastq_golden.json (made by the reference project's own EmbeddedBarcodeGenerator), the
two file-end cases the device code once got wrong, and every seam case's claim -- the byte, the
file end or the buffer size it says it puts at S + d."""

import json
import os

import numpy as np
import pytest

import fastq_reference as F
from conftest import GOLDEN_DIR
from sctools_amd import fastq

FQ_DIR = os.path.join(GOLDEN_DIR, "fastq")


def _golden():
    with open(os.path.join(GOLDEN_DIR, "fastq_golden.json")) as f:
        return json.load(f)


def test_reference_equals_every_golden_case():
    g = _golden()
    assert len(g["cases"]) >= 22
    for case in g["cases"]:
        if "files" in case:
            contents = [open(os.path.join(FQ_DIR, f), "rb").read() for f in case["files"]]
        else:
            contents = [bytes.fromhex(c) for c in case["contents"]]
        tags = [g["tags"][t] for t in case["tags"]]
        ref = F.fastq_reference(contents, [(s, e) for s, e, _, _ in tags], case["mode"])
        got = F.records_of(ref, [(st, qt) for _, _, st, qt in tags], case["mode"])
        want = [[(t, v["str"] if isinstance(v, dict) else bytes.fromhex(v), z) for t, v, z in rec]
                for rec in case["records"]]
        assert got == want, (case["name"], case["mode"])
        # bad_name: the reference project raised after the records before the bad one
        assert (ref.first_bad >= 0) == ("error" in case), case["name"]
        if "error" in case:
            assert ref.first_bad == len(case["records"]) and case["error"]["type"] == "ValueError"


def test_reference_many_files_ending_together_are_one_record():
    """Four unterminated files of a few bytes: one line each, one record."""
    for mode in ("rb", "r"):
        ref = F.fastq_reference([b"@r", b"ACGT", b"+", b"FFFF"], [(0, 16), (1, 3)], mode)
        assert (ref.nrec, ref.first_bad) == (1, -1)
        assert bytes(ref.spans[0][0][0]) == b"ACGT" + bytes(12) and ref.spans[0][1].tolist() == [4]
        assert bytes(ref.spans[1][2][0]) == b"FF" and ref.spans[1][3].tolist() == [2]
        assert F.raw_line_ends([b"@r", b"ACGT", b"+", b"FFFF"], mode) == [2, 6, 7, 11]


def test_reference_cr_file_end_then_lf_file_start_is_two_line_ends():
    """Universal newlines work per file: '\\r' ending one file and '\\n' starting the next are two
    line ends in mode 'r' (the second an empty line)."""
    files = [b"@r\nAC\r", b"\n+\nFF\n"]
    assert F.read_lines(files, "r") == [b"@r\n", b"AC\n", b"\n", b"+\n", b"FF\n"]
    assert F.raw_line_ends(files, "r") == [3, 6, 7, 9, 12]
    assert F.read_lines(files, "rb") == [b"@r\n", b"AC\r", b"\n", b"+\n", b"FF\n"]  # (an unterminated file end)
    ref = F.fastq_reference(files, [(0, 4)], "r")
    assert ref.nrec == 1 and bytes(ref.spans[0][0][0]) == b"AC\n\0" and bytes(ref.spans[0][2][0]) == b"+\n\0\0"
    # the same bytes in one file are one "\r\n"
    assert F.read_lines([b"".join(files)], "r") == [b"@r\n", b"AC\n", b"+\n", b"FF\n"]


def test_reference_encodes_span0_and_refuses_high_bytes_in_text_mode():
    ref = F.fastq_reference([b"@r\nACGTN\n+\nFFFFF\n"], [(0, 6)], "rb")
    # the zero-padded row "ACGTN\n": N ambiguous (bit 0), '\n' invalid (bit 1)
    assert ref.enc[2][2].tolist() == [3] and ref.enc[3][2].tolist() == [0]
    from oracle import oracle as O
    assert int(ref.enc[2][0][0]) == O.two_bit_encode(b"ACGT") << 4 and ref.enc[2][1].tolist() == [2]
    with pytest.raises(UnicodeDecodeError):
        F.fastq_reference([b"@r\nAC\x80T\n+\nFFFF\n"], [(0, 4)], "r")
    assert 2 not in F.fastq_reference([b"@r\n"], [(0, 33)], "rb").enc  # no one-limb code


@pytest.mark.parametrize("family", sorted(F.FAMILIES) + [F.HIGH_FAMILY])
def test_every_seam_case_holds_its_claim(family):
    cs = F.cases(family)
    assert cs and len({c.desc for c in cs}) == len(cs)  # descriptions name the cases
    for c in cs:
        assert c.claims
        F.check_claims(c)
        assert sum(len(x) for x in c.contents) <= 3 * F.TILE + 128 or family == "long"
    assert F.cases(family) is cs  # built once, shared


def test_filler_is_plain():
    """The filler absorbs an offset and holds none of the features."""
    for P in [0, 6, 7, 95, 96, 101, 102, 8191, 8192, 16385]:
        buf = F.filler(P)
        assert len(buf) == P and b"\r" not in buf and max(buf, default=0) < 128
        lines = buf.split(b"\n")
        assert P == 0 or (lines[-1] == b"" and len(lines) % 4 == 1)
        assert all(x.startswith(b"@") for x in lines[0:-1:4]) and all(x == b"+" for x in lines[2:-1:4])
        ref = F.fastq_reference([buf], [(0, 16)], "r")
        assert ref.first_bad == -1 and ref.nrec == (len(lines) - 1) // 4


def test_seam_families_cover_the_seams():
    """The phases the families promise, read back from the claims."""
    def offsets(family, kind):
        return {c.claims[0][1] for c in F.cases(family) if c.claims[0][0] == kind}
    want = {S + d for S in F.SEAMS for d in F.PHASES}
    assert want <= offsets("lf", "byte") and want <= offsets("crlf", "byte") and want <= offsets("ends", "end")
    assert {F.TILE + 15, F.TILE + 16, F.TILE + 17, 2 * F.TILE + 15, 2 * F.TILE + 16, 2 * F.TILE + 17} <= offsets("ends", "end")
    for k, spans in enumerate(F.SPANS):
        fam = ["slices0", "slices1", "slices64", "slices65", "slices_empty"][k]
        assert {F.TILE - j for j in range(max(e for _, e in spans) + 2)} <= offsets(fam, "byte")
    # a file end on the tile seam with no other file end in the tile after it (nor 16 bytes on)
    far = [F.file_ends(c.contents) for c in F.cases("ends") if "then a tile and more" in c.desc]
    assert any(e[0] == F.TILE for e in far) and all(len(e) == 2 and e[1] > 2 * F.TILE + 16 for e in far)
    sizes = {c.claims[0][1] for c in F.cases("buffer_end")}
    assert {0, 1, 3, 15, 16, 17, F.TILE - 1, F.TILE, F.TILE + 1, 2 * F.TILE - 1, 2 * F.TILE, 2 * F.TILE + 1} <= sizes
    # every trailing case drops 1..3 lines; the bad name of a dropped record is not reported
    for c in F.cases("trailing"):
        assert len(F.read_lines(c.contents, "rb")) % 4 in (1, 2, 3), c.desc
    dropped = [c for c in F.cases("bad_names") if "dropped" in c.desc]
    assert dropped and all(F.fastq_reference(c.contents, c.spans, "r").first_bad == -1 for c in dropped)
    two = [c for c in F.cases("bad_names") if "two bad" in c.desc]
    assert two and all(F.fastq_reference(c.contents, c.spans, "r").first_bad >= 0 for c in two)


def _tiles_with_a_line_end(buf):
    a = np.frombuffer(buf, np.uint8)
    return set((np.flatnonzero((a == 10) | (a == 13)) // F.TILE).tolist())


@pytest.mark.parametrize("K", F.COARSE_K)
def test_coarse_pieces_hold_their_claims(K):
    """Every coarse piece: P bytes of whole records ending in '\\n' at byte P - 1 -- the last byte of
    tile K - 1 or the first of tile K -- then exactly the 1..3 complete lines asked for, valid names
    throughout; the long-line variant leaves the tiles on both sides of that byte's tile without a
    line end."""
    for d in (0, 1):
        for tail_lines in (1, 2, 3):
            buf, P = F.coarse_piece(K, d, tail_lines)
            assert P == K * F.TILE + d and (P - 1) // F.TILE == K - 1 + d and (P - 1) % F.TILE == (F.TILE - 1, 0)[d]
            assert buf[P - 1] == 10 and buf[-1] == 10 and b"\r" not in buf and max(buf) < 128
            assert buf[P:].count(b"\n") == tail_lines and len(buf) > P + F.COARSE_LINE * (tail_lines > 1)
            assert buf[:P].count(b"\n") % 4 == 0 and buf[P:P + 1] == b"@"
            ref, whole = F.fastq_reference([buf[:P]], F.SPANS[0], "rb"), F.fastq_reference([buf], F.SPANS[0], "r")
            assert ref.nrec == whole.nrec == buf[:P].count(b"\n") // 4 and ref.first_bad == whole.first_bad == -1
            # records of two lines of COARSE_LINE bytes and little else (the Python reference stays cheap)
            assert P // (2 * F.COARSE_LINE + 100) - 1 <= ref.nrec <= P // (2 * F.COARSE_LINE)
    buf, P = F.coarse_piece(K, 0, 2, long_lines=True)
    assert len(buf) == P + F.COARSE_LONG + F.COARSE_LINE + 1 and buf[P - 1] == 10 and buf[:P].count(b"\n") % 4 == 0
    assert buf[P - F.COARSE_LONG - 1] == 10 and buf[P + F.COARSE_LONG - 1] == 10  # the two long lines
    assert b"\n" not in buf[P - F.COARSE_LONG:P - 1] and b"\n" not in buf[P:P + F.COARSE_LONG - 1]
    t, has = (P - 1) // F.TILE, _tiles_with_a_line_end(buf)
    assert t == K - 1 and t in has and not {t - 1, t + 1} & has
    assert F.fastq_reference([buf[:P]], F.SPANS[0], "r").nrec == F.fastq_reference([buf], F.SPANS[0], "rb").nrec > 0


def test_last_line_end_text_mode():
    """The piece cut in text mode: also after a '\\r' known to stand alone (a byte other than '\\n'
    follows it inside the piece), never after the piece's last byte when that is a '\\r'."""
    def cut(b, text=True):
        a = np.frombuffer(b, np.uint8)
        return fastq._last_line_end(a, a.size, text)
    assert cut(b"ab\rcd") == 3 and cut(b"ab\rcd", False) == 0
    assert cut(b"ab\r") == 0 and cut(b"a\rb\r") == 2
    assert cut(b"ab\r\ncd") == 4 and cut(b"ab\r\n") == 4 and cut(b"a\rb\r\n") == 5
    assert cut(b"a\nb\rc") == 4 and cut(b"a\rb\nc") == 4 and cut(b"\r\r") == 1
    big = np.full(300_000, ord("A"), np.uint8)
    big[5] = 13
    assert fastq._last_line_end(big, big.size, True) == 6 and fastq._last_line_end(big, 6, True) == 0
    big[6] = 10
    assert fastq._last_line_end(big, big.size, True) == 7
