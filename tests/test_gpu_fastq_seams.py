"""The FASTQ extraction (sctools_amd/csrc/fastq.hip) on its own seams: every case of
tests/fastq_reference.py -- one terminator, file end or slice at byte S + d of a 16-byte load, a
thread's 32 bytes, the 8 KiB tile or the buffer end -- in both modes, through every entry form,
against Python's own line reading (fastq_reference).  Exact equality throughout.

Every form runs one count stage (fq_count_kernel, tile_sums_reduce_kernel) and one range stage
(fastq_range_kernel: tile_items, line_spans); they differ in what stands around the two:

indexed  _lib.fastq_extract             an index keeps the count stage's sums; rows laid out by the record count
fused    sct_fastq_extract_fused        both stages in one asynchronous call; rows laid out by a capacity, span 0 encoded
stream   _lib.FastqStream               an index per piece + line_end_kernel's `consumed` from the same sums
drop-in  fastq.EmbeddedBarcodeGenerator the files read in pieces of a few bytes

The coarse pieces (fastq_reference part 3) put a non-final piece's last record end 32 and 1,024
tiles in, where `consumed` and the index's record count come from the sums over blocks of tiles.
"""

import functools

import numpy as np
import pytest

import fastq_reference as F
from test_fastq import _fused

pytestmark = pytest.mark.gpu

MODES = (("rb", 0), ("r", 1))
NAMES = ("seq", "seq_len", "qual", "qual_len")


@functools.lru_cache(maxsize=None)
def _ref(family, i, mode):
    c = F.cases(family)[i]
    return F.fastq_reference(c.contents, c.spans, mode)


def _same(got, ref, what, rows=None):
    """Every span's sequence / quality rows and lengths (the first `rows` records)."""
    n = ref.nrec if rows is None else rows
    assert len(got) == len(ref.spans), what
    for k, (g, r) in enumerate(zip(got, ref.spans)):
        for name, a, b in zip(NAMES, g, r):
            a, b = np.asarray(a)[:n], b[:n]
            assert a.shape == b.shape, (what, k, name, a.shape, b.shape)
            if not np.array_equal(a, b):
                bad = np.flatnonzero((a != b).reshape(n, -1).any(axis=1))
                r0 = int(bad[0])
                raise AssertionError("%s: span %d %s differs in %d records, first %d: got %r, reference %r"
                                     % (what, k, name, bad.size, r0, bytes(a[r0:r0 + 1]), bytes(b[r0:r0 + 1])))


def _each(family):
    for i, c in enumerate(F.cases(family)):
        for mode, text in MODES:
            yield c, b"".join(c.contents), F.file_ends(c.contents), mode, text, _ref(family, i, mode), \
                "%s [%s]" % (c.desc, mode)


def _check_indexed(c, buf, ends, mode, text, ref, what):
    from sctools_amd import _lib
    n, bad, parts = _lib.fastq_extract(buf, ends, c.spans, text)
    assert (n, bad) == (ref.nrec, ref.first_bad), (what, "records, first bad name", (n, bad), (ref.nrec, ref.first_bad))
    _same(parts, ref, what)


def _check_fused(c, buf, ends, mode, text, ref, what, ascii_only=True):
    for kind in (2, 3):
        n, bad, got, enc, na = _fused(buf, ends, c.spans, text, kind=kind, encode=kind in ref.enc)
        assert (n, bad) == (ref.nrec, ref.first_bad), (what, kind, "records, first bad name", (n, bad),
                                                       (ref.nrec, ref.first_bad))
        assert na == 0 or not ascii_only, (what, "non-ASCII status", na)
        _same(got, ref, "%s fused kind %d" % (what, kind))
        if kind in ref.enc:
            for name, a, b in zip(("codes", "gc", "flags"), enc, ref.enc[kind]):
                assert np.array_equal(a, b), (what, "kind %d %s" % (kind, name), a.tolist(), b.tolist())
    n, bad, got, _, na = _fused(buf, ends, c.spans, text, encode=False)
    assert (n, bad) == (ref.nrec, ref.first_bad) and (na == 0 or not ascii_only), (what, "no encode")
    _same(got, ref, what + " fused, no encode")
    if ref.nrec >= 1:  # a capacity one below: the rows below it equal, none at or past it (the helper's guard)
        cap = ref.nrec - 1
        n, bad, got, enc, _ = _fused(buf, ends, c.spans, text, cap=cap, encode=2 in ref.enc)
        assert (n, bad) == (ref.nrec, ref.first_bad), (what, "capacity %d" % cap)
        _same([tuple(x[:cap] for x in g) for g in got], ref, what + " fused, capacity %d" % cap, rows=cap)
        if 2 in ref.enc:
            for a, b in zip(enc, ref.enc[2]):
                assert np.array_equal(a[:cap], b[:cap]), (what, "capacity %d codes" % cap)


def _pieces_reference(c, buf, ends, mode):
    """The two-piece protocol's answers from the reference: the first piece ends at the first line
    end past the case's feature (the last one if none lies past it) and reports the byte after its
    last complete record; the second piece starts there."""
    les = F.raw_line_ends(c.contents, mode)
    at = c.claims[0][1]
    cut = next((e for e in les if e > at), les[-1] if les else 0)
    first = None
    used = 0
    if cut > 0:
        ends1 = [e for e in ends if e < cut] + [cut]
        files1 = F.split(buf[:cut], ends1[:-1])
        ref1 = F.fastq_reference(files1, c.spans, mode)
        les1 = F.raw_line_ends(files1, mode)
        used = les1[4 * ref1.nrec - 1] if ref1.nrec else 0
        first = (cut, ends1, ref1, used)
    rest = buf[used:]
    ends2 = [e - used for e in ends if e > used] or [0]
    ref2 = F.fastq_reference(F.split(rest, ends2[:-1]), c.spans, mode)
    return first, (rest, ends2, ref2)


def _check_stream(c, buf, ends, mode, text, ref, what):
    from sctools_amd import _lib
    st = _lib.FastqStream(c.spans, text, True)
    try:
        n, used, bad, parts = st.chunk(buf, len(buf), ends, True)
        assert (n, used, bad) == (ref.nrec, len(buf), ref.first_bad), (what, "one piece", (n, used, bad))
        _same(parts, ref, what + " one piece")
        first, (rest, ends2, ref2) = _pieces_reference(c, buf, ends, mode)
        n1 = 0
        if first is not None:
            cut, ends1, ref1, want_used = first
            n1, used, bad, parts = st.chunk(buf[:cut], cut, ends1, False)
            assert (n1, used, bad) == (ref1.nrec, want_used, ref1.first_bad), \
                (what, "first piece of %d bytes: records, consumed, first bad" % cut, (n1, used, bad),
                 (ref1.nrec, want_used, ref1.first_bad))
            _same(parts, ref1, what + " first piece of %d bytes" % cut)
        n2, used, bad, parts = st.chunk(rest, len(rest), ends2, True)
        assert (n2, used, bad) == (ref2.nrec, len(rest), ref2.first_bad), (what, "second piece", (n2, used, bad))
        _same(parts, ref2, what + " second piece")
        assert n1 + n2 == ref.nrec, (what, "the pieces' records", n1, n2, ref.nrec)
    finally:
        st.close()


FORMS = {"indexed": _check_indexed, "fused": _check_fused, "stream": _check_stream}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("family", sorted(F.FAMILIES))
def test_fastq_seams(family, form):
    count = 0
    for args in _each(family):
        FORMS[form](*args)
        count += 1
    assert count == 2 * len(F.cases(family))  # every case, both modes


@pytest.mark.parametrize("tiles", (1, 2, 0))
@pytest.mark.parametrize("family", sorted(F.FAMILIES))
def test_fastq_seams_range_sizes(family, tiles):
    """The fused form with fastq_range_kernel's range fixed by ingest_tiles (unset: 8 tiles, under
    which the 8 KiB and 16 KiB seams lie inside a workgroup's range): 1, every 8 KiB seam starts a
    range (line number and file cursor from the tile sums, not carried); 2, the 16 KiB seam starts
    one and the 8 KiB seam is carried; 0, the ranges are sized to the resident grid."""
    from sctools_amd import _lib
    count = 0
    with _lib.tuning(ingest_tiles=tiles):
        assert _lib.tune_get("ingest_tiles") == tiles
        for args in _each(family):
            _check_fused(*args)
            count += 1
    assert _lib.tune_get("ingest_tiles") == -1
    assert count == 2 * len(F.cases(family))  # every case, both modes


@pytest.mark.parametrize("form", sorted(FORMS))
def test_fastq_high_bytes_binary(form):
    """0x80 / 0xFF in sequence and quality lines at the seams, mode 'rb': the bytes arrive in the
    rows unchanged, span 0's flags are the encode reference's (an invalid byte)."""
    for i, c in enumerate(F.cases(F.HIGH_FAMILY)):
        ref = _ref(F.HIGH_FAMILY, i, "rb")
        assert any(int(x[0].max(initial=0)) >= 128 or int(x[2].max(initial=0)) >= 128 for x in ref.spans), c.desc
        args = (c, b"".join(c.contents), F.file_ends(c.contents), "rb", 0, ref, c.desc + " [rb]")
        if form == "fused":
            _check_fused(*args, ascii_only=False)
        else:
            FORMS[form](*args)


def test_fastq_high_bytes_text_is_refused():
    """The same inputs in mode 'r': the reference's reader cannot decode them; the indexed and the
    stream form raise ValueError (ASCII only on the device path), the fused form -- asynchronous, it
    raises nothing -- sets its non-ASCII status word."""
    from sctools_amd import _lib
    for c in F.cases(F.HIGH_FAMILY):
        buf, ends = b"".join(c.contents), F.file_ends(c.contents)
        with pytest.raises(UnicodeDecodeError):
            F.fastq_reference(c.contents, c.spans, "r")
        with pytest.raises(ValueError, match="text-mode FASTQ must be ASCII"):
            _lib.fastq_extract(buf, ends, c.spans, 1)
        st = _lib.FastqStream(c.spans, True, True)
        try:
            with pytest.raises(ValueError, match="text-mode FASTQ must be ASCII"):
                st.chunk(buf, len(buf), ends, True)
        finally:
            st.close()
        assert _fused(buf, ends, c.spans, 1)[4] != 0, c.desc


# ---------------------------------------------------------------- pieces past the coarse levels
@functools.lru_cache(maxsize=None)
def _coarse_ref(K, d, long_lines, mode):
    """The reference of a coarse piece's first P bytes (the same for every tail)."""
    buf, P = F.coarse_piece(K, d, 1, long_lines)
    return F.fastq_reference([buf[:P]], F.SPANS[0], mode)


def _check_coarse(K, d, tail_lines, long_lines=False):
    from sctools_amd import _lib
    buf, P = F.coarse_piece(K, d, tail_lines, long_lines)
    spans = F.SPANS[0]
    for mode, text in MODES:
        ref = _coarse_ref(K, d, long_lines, mode)
        what = "K=%d d=%d, %d tail line(s)%s [%s]" % (K, d, tail_lines, ", long lines" if long_lines else "", mode)
        assert ref.nrec > 0 and ref.first_bad == -1
        st = _lib.FastqStream(spans, text, True)
        try:
            n, used, bad, parts = st.chunk(buf, len(buf), [len(buf)], False)
        finally:
            st.close()
        assert (n, used, bad) == (ref.nrec, P, -1), (what, "records, consumed, first bad", (n, used, bad), (ref.nrec, P, -1))
        _same(parts, ref, what + " non-final piece")
        # the whole buffer through the index route: the unfinished record is dropped, the rows are the same
        whole = F.fastq_reference([buf], spans, mode)
        assert whole.nrec == ref.nrec
        n, bad, parts = _lib.fastq_extract(buf, [len(buf)], spans, text)
        assert (n, bad) == (whole.nrec, whole.first_bad), (what, "indexed: records, first bad name", (n, bad))
        _same(parts, whole, what + " indexed")


@pytest.mark.parametrize("d", (0, 1))
@pytest.mark.parametrize("K", F.COARSE_K)
def test_fastq_consumed_past_blocks_of_tiles(K, d):
    """The last complete record ends on the last byte of tile K - 1 (d = 0) or the first byte of tile
    K (d = 1), K = one block of the middle level and one of the top level; one to three complete
    lines of an unfinished record follow.  `consumed` of the non-final piece is exactly P."""
    for tail_lines in (1, 2, 3):
        _check_coarse(K, d, tail_lines)


@pytest.mark.parametrize("K", F.COARSE_K)
def test_fastq_consumed_between_tiles_without_a_line_end(K):
    """The lines on both sides of the last record end are 20,000 bytes: the tiles before and after
    the tile that holds it count no terminator."""
    _check_coarse(K, 0, 2, long_lines=True)


# ---------------------------------------------------------------- the drop-in, files in tiny pieces
def _dropin_cases():
    """File ends, "\\r\\n" and '\\r' line ends, '\\r'-only files and trailing records, at the load
    seam (the pieces move every later seam anyway)."""
    out = []
    for family in ("ends", "crlf", "trailing"):
        for i, c in enumerate(F.cases(family)):
            if sum(len(x) for x in c.contents) < 600 and (c.claims[0][1] in (F.LOAD - 1, F.LOAD, F.LOAD + 1)
                                                         or "cluster" in c.desc or "empty file" in c.desc):
                out.append((family, i, c))
    out += [("cr_only", i, c) for i, c in enumerate(F.cases("cr_only"))]
    return out


@pytest.mark.parametrize("chunk", [7, 64, 333])
def test_fastq_seams_dropin_small_pieces(tmp_path, monkeypatch, chunk):
    from sctools_amd import fastq
    monkeypatch.setattr(fastq, "CHUNK_BYTES", chunk)
    todo = _dropin_cases()
    assert len(todo) > 60 and {f for f, _, _ in todo} == {"ends", "crlf", "trailing", "cr_only"}
    for j, (family, i, c) in enumerate(todo):
        paths = []
        for k, data in enumerate(c.contents):
            p = tmp_path / ("c%d_%d.fastq" % (j, k))
            p.write_bytes(data)
            paths.append(str(p))
        tags = [("S%d" % k, "Q%d" % k) for k in range(len(c.spans))]
        ebs = [fastq.EmbeddedBarcode(s, e, st, qt) for (s, e), (st, qt) in zip(c.spans, tags)]
        for mode, _ in MODES:
            ref, what = _ref(family, i, mode), "%s [%s] pieces of %d" % (c.desc, mode, chunk)
            gen = fastq.EmbeddedBarcodeGenerator(ebs, paths, mode)
            want = F.records_of(ref, tags, mode)
            if ref.first_bad >= 0:
                got = []
                with pytest.raises(ValueError, match="fastq name must start with @"):
                    for rec in gen:
                        got.append(rec)
                assert got == want, what
                with pytest.raises(ValueError, match="fastq name must start with @"):
                    len(gen)
                with pytest.raises(ValueError, match="fastq name must start with @"):
                    gen.extract_arrays()
                continue
            assert list(gen) == want, what
            assert len(gen) == ref.nrec, what
            arr = gen.extract_arrays()
            for (st, qt), (s, e), (seq, slen, qual, qlen) in zip(tags, c.spans, ref.spans):
                for tag, rows, lens in ((st, seq, slen), (qt, qual, qlen)):
                    assert arr[tag][0].dtype == np.dtype("S%d" % (e - s)) and arr[tag][0].shape == (ref.nrec,), what
                    assert arr[tag][0].tobytes() == rows.tobytes() and np.array_equal(arr[tag][1], lens), (what, tag)
