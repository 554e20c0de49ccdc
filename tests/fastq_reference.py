"""A plain reading of FASTQ embedded-barcode extraction, and inputs that put one feature on one
seam of the device code (sctools_amd/csrc/fastq.hip).

Part 1, fastq_reference: the lines of every file as Python's own io readers give them (the way
reader.Reader reads: one file at a time, 'rb' bytes lines, 'r' universal newlines), four lines a
record, line[s:e] slices.  No newline is split here and nothing of the device layout is known.

Part 2, the seam cases: deterministic (contents, description, claims) with one feature -- a
terminator, a file end, a slice's first byte -- at byte S + d of the concatenated files.  Every
claim is checked on the CPU (tests/test_fastq_reference_host.py) before a GPU test relies on it.

Part 3, the coarse pieces: whole records up to a tile seam 32 or 1,024 tiles in, then the first
lines of a record that never ends (their claims are checked on the CPU in the same place).
"""

import io
from collections import namedtuple

import numpy as np

import encode_reference as E

# ---------------------------------------------------------------- part 1: the reference
Ref = namedtuple("Ref", "nrec first_bad spans enc")


def read_lines(contents, mode):
    """The line streams of the files, concatenated; bytes lines ('r': as the text reader gives them)."""
    lines = []
    for c in contents:
        if mode == "rb":
            lines += io.BytesIO(c).readlines()
        else:
            text = io.TextIOWrapper(io.BytesIO(c), encoding="ascii", newline=None)
            lines += [s.encode("ascii") for s in text.readlines()]
    return lines


def raw_line_ends(contents, mode):
    """The offset just past every line in the concatenated bytes (newline='' keeps the text
    reader's line ends untranslated, so the lengths are the files' own)."""
    ends, base = [], 0
    for c in contents:
        if mode == "rb":
            raw = io.BytesIO(c).readlines()
        else:
            text = io.TextIOWrapper(io.BytesIO(c), encoding="ascii", newline="")
            raw = [s.encode("ascii") for s in text.readlines()]
        assert b"".join(raw) == c
        for ln in raw:
            base += len(ln)
            ends.append(base)
    assert len(ends) == len(read_lines(contents, mode))
    return ends


def fastq_reference(contents, spans, mode):
    """Ref(nrec, first_bad, [(seq rows (nrec, e - s) uint8 zero-padded, seq lengths int32, qual rows,
    qual lengths) per span], {2: (codes, gc, flags), 3: ...} of span 0's sequence rows where they
    fit one limb)."""
    lines = read_lines(contents, mode)
    nrec = len(lines) // 4
    first_bad = next((r for r in range(nrec) if not lines[4 * r].startswith(b"@")), -1)
    out = []
    for s, e in spans:
        w = e - s
        part = []
        for which in (1, 3):
            rows = np.zeros((nrec, w), np.uint8)
            lens = np.zeros(nrec, np.int32)
            for r in range(nrec):
                x = lines[4 * r + which][s:e]
                rows[r, :len(x)] = np.frombuffer(x, np.uint8)
                lens[r] = len(x)
            part += [rows, lens]
        out.append(tuple(part))
    enc = {}
    if spans:
        w0 = spans[0][1] - spans[0][0]
        for kind in (2, 3):
            if kind * w0 <= 64:
                codes, gc, flags = E.encode(kind, out[0][0], 1)
                enc[kind] = (codes[:, 0], gc, flags)
    return Ref(nrec, first_bad, out, enc)


# ---------------------------------------------------------------- part 2: seam cases
# The seams of the device code: a 16-byte load, a thread's 32 bytes, the 8 KiB tile and its double.
LOAD, THREAD, TILE = 16, 32, 8192
SEAMS = (LOAD, THREAD, TILE, 2 * TILE)
PHASES = (-2, -1, 0, 1, 2)
SPANS = ([(0, 16), (16, 26), (3, 9)], [(1, 10), (0, 8), (2, 14), (0, 33)], [(0, 64)], [(0, 65)], [(5, 5)])

# claims: ("byte", offset, value) the buffer holds value there; ("end", offset) a file ends there;
# ("n", size) the buffer's size
Case = namedtuple("Case", "contents desc claims spans")


def seq_of(i, L):
    return bytes(b"ACGT"[(i + j + (j >> 2)) & 3] for j in range(L))


def qual_of(i, L):
    return bytes(70 + (7 * i + j) % 30 for j in range(L))


def record(i, L=30, eol=b"\n", extra=0, name=None, eols=None):
    """The four lines of record i; eols: {line kind: its own line end}."""
    eols = eols or {}
    body = [(b"@" + b"n" * extra) if name is None else name, seq_of(i, L), b"+", qual_of(i, L)]
    return [b + eols.get(q, eol) for q, b in enumerate(body)]


def filler(P, i0=100):
    """Exactly P bytes (0 or >= 6) of whole '\\n'-ended records in one file: plain reads, valid
    names, no '\\r', no high byte."""
    assert P == 0 or P >= 6, P
    out, i = [], i0
    while P:
        R = 96 if P >= 102 else P
        L = min(30, (R - 6) // 2)
        out += record(i, L, extra=R - 6 - 2 * L)
        P -= R
        i += 1
    return b"".join(out)


def tail_records(k, L=30):
    return b"".join(b"".join(record(900 + j, L)) for j in range(k))


def split(buf, cuts):
    """The files of buf cut at `cuts` (non-decreasing; a repeated cut is an empty file)."""
    assert list(cuts) == sorted(cuts) and all(0 <= c <= len(buf) for c in cuts)
    edges = [0] + list(cuts) + [len(buf)]
    return [buf[a:b] for a, b in zip(edges, edges[1:])]


def file_ends(contents):
    return np.cumsum([len(c) for c in contents]).tolist()


def placed(desc, target, make, tail=2, spans=SPANS[0], more_claims=()):
    """make(x) -> (blob starting a record, k, cuts inside blob, value): blob[k] is the claimed byte
    (value None: a file ends at k); x more bytes go in front of k when the filler cannot absorb the
    offset.  The case has it at `target`."""
    blob, k, cuts, value = make(0)
    P = target - k
    if 0 < P < 6:
        blob, k, cuts, value = make(P)
        P = target - k
    buf = filler(P) + blob + tail_records(tail)
    claims = [("byte", target, value) if value is not None else ("end", target)]
    claims += [(c[0], c[1] + P) + tuple(c[2:]) for c in more_claims]
    return Case(split(buf, [P + c for c in cuts]), "%s at %d" % (desc, target), claims, spans)


def _short(S):
    return S < TILE


def family_lf():
    out = []
    for S in SEAMS:
        for d in PHASES:
            for q in range(4):
                def make(x, q=q, L=4 if _short(S) else 30):
                    ls = record(1, L, extra=x)
                    return b"".join(ls), len(b"".join(ls[:q + 1])) - 1, [], 10
                out.append(placed("lf of line kind %d, S=%d d=%+d" % (q, S, d), S + d, make))
    return out


CR_EOLS = (("crlf", b"\r\n", 0), ("cr", b"\r", 0), ("crcrlf", b"\r\r\n", 0), ("lfcr", b"\n\r", 1),
           ("crlfcrlf", b"\r\n\r\n", 0))


def family_crlf():
    out = []
    for S in SEAMS:
        full = S in (LOAD, TILE)
        L = 3 if _short(S) else 10
        for d in PHASES:
            for name, eol, at in CR_EOLS:
                kinds = range(4) if name in ("crlf", "cr") else (1, 3)
                if not full:
                    kinds = (1,) if name in ("crlf", "cr") else ()
                for q in kinds:
                    def make(x, q=q, eol=eol, at=at):
                        ls = record(2, L, extra=x, eols={q: eol})
                        return b"".join(ls), len(b"".join(ls[:q + 1])) - len(eol) + at, [], 13
                    out.append(placed("%s of line kind %d, S=%d d=%+d" % (name, q, S, d), S + d, make))

            def make_all(x):  # three records of "\r\n" lines; the claim is the first sequence line's '\r'
                ls = record(3, L, b"\r\n", extra=x)
                rest = b"".join(b"".join(record(4 + j, 30, b"\r\n")) for j in range(2))
                return b"".join(ls) + rest, len(ls[0]) + L, [], 13
            out.append(placed("all-crlf records, S=%d d=%+d" % (S, d), S + d, make_all))
    return out


def family_ends():
    """A file end at S + d."""
    out = []

    def add(desc, E, make, **kw):
        out.append(placed("file end: %s" % desc, E, make, **kw))

    for S in SEAMS:
        L = 3 if _short(S) else 30
        for d in PHASES:
            E, tag = S + d, "S=%d d=%+d" % (S, d)
            for q in range(4):  # (after a name or a '+' line the next file's first line is a sliced one)
                def lf_term(x, q=q):  # ends after line kind q's '\n'
                    ls = record(5, L, extra=x)
                    k = len(b"".join(ls[:q + 1]))
                    return b"".join(ls), k, [k], None
                add("'\\n'-terminated after line kind %d, %s" % (q, tag), E, lf_term)

                def unterm(x, q=q):  # ends after line kind q's content: no terminator
                    ls = record(6, L, extra=x, eols={q: b""})
                    k = len(b"".join(ls[:q + 1]))
                    return b"".join(ls), k, [k], None
                add("unterminated after line kind %d, %s" % (q, tag), E, unterm)

                def cr_end(x, q=q):  # the file's last byte is '\r'
                    ls = record(7, L, extra=x, eols={q: b"\r"})
                    k = len(b"".join(ls[:q + 1]))
                    return b"".join(ls), k, [k], None
                add("ends in '\\r' after line kind %d, %s" % (q, tag), E, cr_end)

                def cr_lf(x, q=q):  # '\r' ends the file, the next file starts with '\n'
                    ls = record(8, L, extra=x, eols={q: b"\r\n"})
                    k = len(b"".join(ls[:q + 1])) - 1
                    return b"".join(ls), k, [k], None
                add("'\\r' | '\\n' after line kind %d, %s" % (q, tag), E, cr_lf)

            for name, eol in (("terminated", b"\n"), ("unterminated", b"")):
                for copies in (2, 3):  # one or two empty files after a file that ends at E
                    def empties(x, eol=eol, copies=copies):
                        ls = record(9, L, extra=x, eols={3: eol})
                        k = len(b"".join(ls))
                        return b"".join(ls), k, [k] * copies, None
                    add("%d empty file(s) after a %s file, %s" % (copies - 1, name, tag), E, empties)

    # '\r' | '\n' exactly on a tile seam with more than a tile of records after it: the tile that starts
    # with the '\n' holds no other file end, so the seam's own end is all that marks it
    for d in (-1, 0, 1):
        for q in range(4):
            def cr_lf_far(x, q=q):
                ls = record(8, 30, extra=x, eols={q: b"\r\n"})
                k = len(b"".join(ls[:q + 1])) - 1
                return b"".join(ls), k, [k], None
            add("'\\r' | '\\n' after line kind %d, S=%d d=%+d, then a tile and more" % (q, TILE, d), TILE + d,
                cr_lf_far, tail=130)
    # empty files first and last
    body = filler(300)
    for name, cuts in (("first", [0]), ("first two", [0, 0]), ("last", [300]), ("first and last", [0, 300, 300])):
        c = split(body, cuts)
        out.append(Case(c, "file end: empty file %s" % name, [("end", cuts[0]), ("n", 300)], SPANS[0]))
    # the last file end = n on a tile boundary
    for n in (TILE, 2 * TILE):
        for name, fin in (("'\\n'", b"\n"), ("no terminator", b""), ("'\\r'", b"\r")):
            buf = filler(n - 96) + b"".join(record(10, 30, extra=31 - len(fin), eols={3: fin}))
            out.append(Case([buf], "file end: the buffer ends at %d with %s" % (n, name),
                            [("n", n), ("end", n)], SPANS[0]))
    # the tile's file-end window: ends at t0 + TILE + 15, + 16, + 17
    for t0 in (0, TILE):
        for d in (15, 16, 17):
            E = t0 + TILE + d
            for q in (1, 3):
                def lf_term(x, q=q):
                    ls = record(11, 30, extra=x)
                    k = len(b"".join(ls[:q + 1]))
                    return b"".join(ls), k, [k], None
                add("'\\n'-terminated after line kind %d, t0=%d + TILE + %d" % (q, t0, d), E, lf_term)

                def unterm(x, q=q):
                    ls = record(12, 30, extra=x, eols={q: b""})
                    k = len(b"".join(ls[:q + 1]))
                    return b"".join(ls), k, [k], None
                add("unterminated after line kind %d, t0=%d + TILE + %d" % (q, t0, d), E, unterm)
    # several unterminated files ending within a few bytes; the cluster's first byte at `first`
    clusters = (("four-file record", b"", [b"@r", b"ACGT", b"+", b"FFFF"]),
                ("four one-byte files", b"", [b"@", b"A", b"+", b"F"]),
                ("three files", b"@r\n", [b"ACGT", b"+", b"FFFF"]),
                ("two files", b"@r\nACGT\n", [b"+", b"FFFF"]))
    starts = [(LOAD + 1, "inside one load"), (LOAD - 3, "across a load seam"), (THREAD - 3, "across a thread seam"),
              (TILE + 1, "inside one load"), (2 * TILE - 3, "across a tile seam")]
    starts += [(TILE - j, "across a tile seam") for j in range(1, 12)]
    for first, where in starts:
        for name, lead, files in clusters:
            def make(x, lead=lead, files=files):
                assert x == 0
                cuts = np.cumsum([len(lead)] + [len(f) for f in files]).tolist()
                return lead + b"".join(files), len(lead), cuts, files[0][0]
            if first - len(lead) < 6:
                continue
            c = placed("cluster of %s %s" % (name, where), first, make, tail=2)
            out.append(c._replace(claims=c.claims + [("end", first + len(files[0]))]))
    return out


def family_long():
    out = []

    def rec_with(which, n, fin=b"\n"):
        ls = record(13, 30)
        fill = {0: b"n", 1: None, 2: b"p", 3: None}[which]
        if fill:
            ls[which] = ls[which][:1] + fill * (n - 1) + fin
        else:
            ls[which] = (seq_of(13, n) if which == 1 else qual_of(13, n)) + fin
        return ls

    def add(desc, ls, which, tail=2, cut=None):
        head = filler(96)
        k = len(head) + len(b"".join(ls[:which + 1])) - 1
        buf = head + b"".join(ls) + tail_records(tail)
        out.append(Case(split(buf, [cut + len(head)] if cut is not None else []), "long line: " + desc,
                        [("byte", k, buf[k])], SPANS[0]))

    for n in (8190, 8191, 8192, 8193, 8194, 2 * TILE + 5, 40000):
        for which in (1, 3):
            add("line kind %d of %d bytes" % (which, n), rec_with(which, n), which)
    for n in (2 * TILE + 5, 40000):
        for which in (0, 2):
            add("line kind %d of %d bytes" % (which, n), rec_with(which, n), which)
    for which in (1, 3):
        ls = rec_with(which, 40000, b"")
        add("unterminated last line of a file, kind %d" % which, ls, which, cut=len(b"".join(ls[:which + 1])))
    add("the buffer's unterminated last line", rec_with(3, 40000, b""), 3, tail=0)
    add("the buffer's last line", rec_with(3, 40000), 3, tail=0)
    return out


def family_slices(set_index):
    """A sequence line, then a quality line, starting at TILE - j: every slice's first byte passes
    the seam."""
    spans = SPANS[set_index]
    out = []
    for j in range(max(e for _, e in spans) + 2):
        for q in (1, 3):
            def make(x, q=q):
                ls = record(14 + j, 70, extra=x)
                k = len(b"".join(ls[:q]))
                return b"".join(ls), k, [], ls[q][0]
            out.append(placed("line kind %d starts at TILE - %d" % (q, j), TILE - j, make, spans=spans))
    return out


def family_short_reads():
    """Reads of 0 .. max_end + 1 bytes whose line starts 8 bytes before the tile seam: the '\\n'
    falls on every byte of every slice (and before it, and on the read's first byte)."""
    out = []
    for spans in SPANS[:3]:
        for L in range(max(e for _, e in spans) + 2):
            def make(x):
                ls = record(40 + L, L, extra=x)
                return b"".join(ls), len(ls[0]), [], ls[1][0]
            out.append(placed("read of %d bytes, spans %s, line start" % (L, spans), TILE - 8, make, spans=spans))
    return out


def family_buffer_end():
    out = []
    for fin in (b"", b"\n", b"\r\n"):
        for r in range(25):
            buf = filler(192) + b"".join(record(15, 26 + r, eols={3: fin}))
            out.append(Case([buf], "buffer end: the last slice ends %d bytes before the line end %r" % (r, fin),
                            [("n", len(buf))], SPANS[0]))
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        out.append(Case([filler(n)], "buffer end: n = %d" % n, [("n", n), ("byte", n - 1, 10)], SPANS[0]))
        out.append(Case([filler(n + 1)[:-1]], "buffer end: n = %d, no final newline" % n, [("n", n)], SPANS[0]))
    tiny = b"@r\nACGT\n+\nFFFF\n@s\nAC"
    for n in (0, 1, 3, 15, 16, 17):
        out.append(Case([tiny[:n]], "buffer end: n = %d" % n, [("n", n)], SPANS[0]))
    for name, buf in (("only '\\n'", b"\n" * 9), ("only \"\\r\\n\"", b"\r\n" * 5), ("only '\\r'", b"\r" * 7),
                      ("three lines", b"@r\nACGT\n+\n"), ("three lines, unterminated", b"@r\nACGT\n+"),
                      ("one unterminated line", b"@r")):
        out.append(Case([buf], "buffer end: " + name, [("n", len(buf))], SPANS[0]))
    return out


def family_trailing():
    """1 .. 3 leftover lines after the last record, the first one's '\\n' at S + d, the buffer
    ending with them: the last tiles hold terminators that end no record's line."""
    out = []
    left = [b"@t\n", b"ACGT\n", b"+\n"]
    for S in (LOAD, TILE, 2 * TILE):
        for d in PHASES:
            for k in (1, 2, 3):
                for fin in ((b"\n", b"") if k > 1 else (b"\n",)):
                    def make(x, k=k, fin=fin):
                        assert x == 0
                        blob = b"".join(left[:k])
                        return blob[:len(blob) - 1] + fin, 2, [], 10
                    if S + d - 2 < 6:
                        continue
                    out.append(placed("%d leftover line(s)%s, S=%d d=%+d" % (k, "" if fin else " unterminated", S, d),
                                      S + d, make, tail=0))
    return out


def family_bad_names():
    out = []
    good = tail_records(2)
    out.append(Case([b"r0\nACGT\n+\nFFFF\n" + good], "bad name in record 0", [("byte", 0, ord("r"))], SPANS[0]))
    for S in (TILE, 2 * TILE):
        for d in PHASES:
            def make(x):
                assert x == 0
                return b"".join(record(16, 30, name=b"x16")), 0, [], ord("x")
            out.append(placed("bad name starting at S=%d d=%+d" % (S, d), S + d, make))

    def dropped(x):
        return b"bad\nACGT\n", 0, [], ord("b")
    for S in (LOAD, TILE):
        out.append(placed("bad name in the dropped trailing record, S=%d" % S, S, dropped, tail=0))
    # two bad names in different tiles (the lower one is reported), in either order of the tiles' work
    for first in (96, TILE - 96):
        buf = filler(first) + b"".join(record(17, 30, name=b"y")) + filler(TILE)
        k2 = len(buf)
        buf += b"".join(record(18, 30, name=b"z")) + tail_records(1)
        out.append(Case([buf], "two bad names, at %d and %d" % (first, k2),
                        [("byte", first, ord("y")), ("byte", k2, ord("z"))], SPANS[0]))
    # a bad name after a file's unterminated end and after a '\r' that ends a file
    for name, fin in (("an unterminated file end", b""), ("a '\\r' file end", b"\r")):
        def make(x, fin=fin):
            ls = record(19, 30, extra=x, eols={3: fin})
            k = len(b"".join(ls))
            return b"".join(ls) + b"".join(record(20, 30, name=b"w")), k, [k], ord("w")
        c = placed("bad name after %s" % name, TILE, make)
        out.append(c._replace(claims=c.claims + [("end", TILE)]))
    return out


def family_high_bytes():
    """0x80 / 0xFF in a sequence or a quality line at S + d ('rb' keeps them; 'r' refuses the input)."""
    out = []
    for S in (LOAD, TILE):
        L = 4 if _short(S) else 30
        for d in PHASES:
            for q in (1, 3):
                for val in (0x80, 0xFF):
                    def make(x, q=q, val=val):
                        ls = record(21, L, extra=x)
                        ls[q] = ls[q][:3] + bytes([val]) + ls[q][4:]
                        return b"".join(ls), len(b"".join(ls[:q])) + 3, [], val
                    out.append(placed("byte 0x%02X in line kind %d, S=%d d=%+d" % (val, q, S, d), S + d, make))
    return out


def family_cr_only():
    """Files whose only line end is a lone '\\r' (one line in 'rb')."""
    body = b"".join(b"".join(record(30 + j, 20, b"\r")) for j in range(6))
    out = []
    for name, buf, cuts in (("one file", body, []), ("unterminated", body[:-1], []), ("cut inside a line", body, [30]),
                            ("cut after a '\\r'", body, [body.index(b"\r") + 1]), ("then '\\n' records", body + tail_records(2), [])):
        out.append(Case(split(buf, cuts), "'\\r'-only file: " + name, [("byte", body.index(b"\r"), 13)], SPANS[0]))
    return out


def records_of(ref, tags, mode):
    """The drop-in's records: [(sequence_tag, slice, 'Z'), (quality_tag, slice, 'Z'), ...] per record
    before the first bad name (str fields in mode 'r')."""
    out = []
    for r in range(ref.nrec if ref.first_bad < 0 else ref.first_bad):
        rec = []
        for (st, qt), (seq, slen, qual, qlen) in zip(tags, ref.spans):
            s, q = bytes(seq[r, :slen[r]]), bytes(qual[r, :qlen[r]])
            if mode == "r":
                s, q = s.decode("ascii"), q.decode("ascii")
            rec += [(st, s, "Z"), (qt, q, "Z")]
        out.append(rec)
    return out


FAMILIES = {
    "cr_only": family_cr_only,
    "lf": family_lf,
    "crlf": family_crlf,
    "ends": family_ends,
    "long": family_long,
    "slices0": lambda: family_slices(0),
    "slices1": lambda: family_slices(1),
    "slices64": lambda: family_slices(2),
    "slices65": lambda: family_slices(3),
    "slices_empty": lambda: family_slices(4),
    "short_reads": family_short_reads,
    "buffer_end": family_buffer_end,
    "trailing": family_trailing,
    "bad_names": family_bad_names,
}
HIGH_FAMILY = "high_bytes"  # its text-mode half is refused by the extraction: tested on its own

_cache = {}


def cases(family):
    if family not in _cache:
        _cache[family] = family_high_bytes() if family == HIGH_FAMILY else FAMILIES[family]()
    return _cache[family]


# ---------------------------------------------------------------- part 3: pieces past the coarse levels
# The device code sums its tiles' line counts over blocks of 32 and of 1,024 tiles; a non-final
# piece's `consumed` is found through those sums.  A coarse piece is P = K * TILE + d bytes of whole
# records -- so the last complete record's final '\n' is the last byte of tile K - 1 (d = 0) or the
# first of tile K (d = 1) -- and then 1..3 complete lines of a record that never ends.  Lines of
# 4,000 bytes keep the Python reference at about a thousand records per 8 MiB.
COARSE_K = (32, 1024)
COARSE_LINE, COARSE_LONG = 4000, 20000
_long = []


def _long_records():
    if not _long:
        _long.extend(b"".join(record(50 + i, COARSE_LINE)) for i in range(5))
    return _long


def coarse_piece(K, d, tail_lines, long_lines=False):
    """(buf, P).  long_lines: the last complete record's quality line and the unfinished record's
    name line are COARSE_LONG bytes each (with their '\\n'), so the tiles before and after the one
    that holds byte P - 1 hold no terminator."""
    P = K * TILE + d
    recs = _long_records()
    base = len(recs[0])
    last = record(60, COARSE_LINE)
    if long_lines:
        last[3] = qual_of(60, COARSE_LONG - 1) + b"\n"
    room = len(b"".join(last))
    n = (P - room) // base
    body = b"".join(recs[i % len(recs)] for i in range(n))
    last[0] = b"@" + b"n" * (P - len(body) - room) + b"\n"  # the name line sized to reach P
    tail = record(61, COARSE_LINE)
    if long_lines:
        tail[0] = b"@" + b"m" * (COARSE_LONG - 2) + b"\n"
    return body + b"".join(last) + b"".join(tail[:tail_lines]), P


def check_claims(case):
    buf = b"".join(case.contents)
    ends = file_ends(case.contents)
    for c in case.claims:
        if c[0] == "byte":
            assert 0 <= c[1] < len(buf) and buf[c[1]] == c[2], (case.desc, c, buf[max(0, c[1] - 4):c[1] + 4])
        elif c[0] == "end":
            assert c[1] in ends, (case.desc, c, ends)
        else:
            assert c[0] == "n" and len(buf) == c[1], (case.desc, c, len(buf))
