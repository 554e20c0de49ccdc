"""Whitelist ingest (sctools_amd/csrc/lines.hip, tile_prefix.h) on its own seams: every case of
tests/whitelist_reference.py -- a '\\n', an empty line, a split line, a long line, the file's end
or a capacity at byte S + d of a lane's 16 bytes, a wave's 1 KiB, the 4 KiB sub-tile, the 16 KiB
tile and a workgroup's range of tiles -- against Python's own line reading and the encode
reference.  Exact equality throughout; every limb of every line is compared.

The knobs move the seams of the launch, never a result:
ingest_tiles   tiles per workgroup of whitelist_fused_kernel (unset: one range per resident slot,
               one tile each at these sizes; 2 and 3: the range loop carries the line number and
               the last line end from tile to tile; 64: one workgroup walks the whole buffer)
ingest_direct  unset: every workgroup sums the tiles before its own (tile_prefix_direct);
               0: tile_sums_reduce_kernel and the coarse sums (tile_prefix)
ingest_spec    0: a file of 16-base lines takes the count and encode passes too

The coarse pieces pass 1,024 tiles (blocks of 32 and of 1,024 tiles in the sums, five words per
thread in tile_prefix_direct) and every resident grid (wl_count_kernel strides; the default range
is more than one tile).
"""

import ctypes
import functools
from collections import Counter

import numpy as np
import pytest

import whitelist_reference as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TILES = (None, 1, 2, 3, 64)
DIRECT = (None, 0)
KINDS = ((2, 1), (3, 1), (2, 2))
GUARD = 64  # rows past the last line: nothing may be written there
FILL = {"codes": -5, "starts": -6, "lens": -7, "gc": 0xEE, "flags": 77}


@functools.lru_cache(maxsize=None)
def _lines(family, i):
    return W.read_lines(W.cases(family)[i].data)


@functools.lru_cache(maxsize=None)
def _enc(family, i, kind, words):
    return W.encode_lines(W.cases(family)[i].data, _lines(family, i), kind, words)


def _upload(data):
    import torch
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


def _encode(d_buf, nbytes, kind, words, cap, rows):
    """sct_whitelist_encode into `rows` rows of fill; (count, longest, {name: host array})."""
    import torch
    from sctools_amd import _lib
    out = {"codes": torch.full((rows * words,), FILL["codes"], dtype=torch.int64, device="cuda"),
           "starts": torch.full((rows,), FILL["starts"], dtype=torch.int64, device="cuda"),
           "lens": torch.full((rows,), FILL["lens"], dtype=torch.int32, device="cuda"),
           "gc": torch.full((rows,), FILL["gc"], dtype=torch.uint8, device="cuda"),
           "flags": torch.full((rows,), FILL["flags"], dtype=torch.uint8, device="cuda")}
    d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_mx = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().sct_whitelist_encode(
        d_buf.data_ptr(), nbytes, kind, words, cap, out["codes"].data_ptr(), out["starts"].data_ptr(),
        out["lens"].data_ptr(), out["gc"].data_ptr(), out["flags"].data_ptr(), d_n.data_ptr(), d_mx.data_ptr(), None))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host["codes"] = host["codes"].view(np.uint64).reshape(rows, words)
    return int(d_n.item()), int(d_mx.item()), host


def _first_bad(a, b):
    bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
    return "%d rows differ, first %d: got %r, reference %r" % (bad.size, bad[0], a[bad[0]].tolist(), b[bad[0]].tolist())


def _same(got, ref, enc, cap, words, what):
    """The count, the longest line, every row below the capacity, and the fill at and past it."""
    n, mx, out = got
    assert (n, mx) == (ref.n, ref.maxlen), (what, "lines, longest line", (n, mx), (ref.n, ref.maxlen))
    m = min(cap, ref.n)
    want = {"starts": ref.starts, "lens": ref.lens, "codes": enc.codes, "gc": enc.gc, "flags": enc.flags}
    for name, w in want.items():
        assert np.array_equal(out[name][:m], w[:m]), "%s: %s: %s" % (what, name, _first_bad(out[name][:m], w[:m]))
        fill = np.array(FILL[name], np.int64).astype(np.uint64) if name == "codes" else FILL[name]
        assert (out[name][m:] == fill).all(), "%s: %s: a row at or past the capacity %d was written" % (what, name, m)


def _settings(case):
    """(knobs, label) of one case: ingest_tiles x ingest_direct, and for files of 16-base lines
    ingest_spec 0 and 1."""
    stride = W.claim(case, "stride")
    specs = (None, 0) if stride and stride[0][1] == 17 else (None,)
    for spec in specs:
        for direct in DIRECT:
            for tiles in TILES:
                knobs = {k: v for k, v in (("ingest_tiles", tiles), ("ingest_direct", direct), ("ingest_spec", spec))
                         if v is not None}
                yield knobs, "tiles %s direct %s spec %s" % (tiles, direct, spec)


def _check_case(family, i, kind, words):
    from sctools_amd import _lib
    case = W.cases(family)[i]
    ref, enc = _lines(family, i), _enc(family, i, kind, words)
    caps = [x[1] for x in W.claim(case, "cap")] or [ref.n]
    d_buf = _upload(case.data)
    runs = 0
    for cap in caps:
        first = None
        for knobs, label in _settings(case):
            with _lib.tuning(**knobs):
                got = _encode(d_buf, len(case.data), kind, words, cap, ref.n + GUARD)
            what = "%s [kind %d, %d limb(s), capacity %d, %s]" % (case.desc, kind, words, cap, label)
            _same(got, ref, enc, cap, words, what)
            if first is None:
                first = got
            else:  # byte for byte what the first setting gave, the rows past the capacity included
                assert got[:2] == first[:2] and all(a.tobytes() == first[2][k].tobytes() for k, a in got[2].items()), what
            runs += 1
    return runs


@pytest.mark.parametrize("kind,words", KINDS)
@pytest.mark.parametrize("family", sorted(W.FAMILIES))
def test_whitelist_seams(family, kind, words):
    cs = W.cases(family)
    runs = sum(_check_case(family, i, kind, words) for i in range(len(cs)))
    spec = sum(1 for c in cs if W.claim(c, "stride") and W.claim(c, "stride")[0][1] == 17)
    assert runs == (len(cs) + spec) * len(TILES) * len(DIRECT)  # every case under every setting


def test_whitelist_gc_saturates():
    """Lines of up to 300 G / C bases in ten limbs, over the first tile seam: gc stops at 255."""
    assert _enc(W.GC_FAMILY, 0, 2, 10).gc.max() == 255
    assert _check_case(W.GC_FAMILY, 0, 2, 10) == len(TILES) * len(DIRECT)
    assert _check_case(W.GC_FAMILY, 0, 2, 9) == len(TILES) * len(DIRECT)  # the 300-base lines: flag 4


# ---------------------------------------------------------------- the coarse pieces
def _check_coarse(ntiles, settings):
    from sctools_amd import _lib
    data = W.coarse_piece(ntiles)
    ref = W.check_coarse(data, ntiles)
    enc = W.encode_lines(data, ref, 2, 1)
    d_buf = _upload(data)
    for knobs in settings:
        for cap in (ref.n, ref.n - 1):
            with _lib.tuning(**knobs):
                got = _encode(d_buf, len(data), 2, 1, cap, ref.n + GUARD)
            _same(got, ref, enc, cap, 1, "%d tiles [%s, capacity %d]" % (ntiles, knobs or "defaults", cap))
    return data, ref, d_buf


def test_whitelist_past_blocks_of_tiles():
    """Piece (a), 1,058 tiles: tile_prefix_direct sums five words per thread; with ingest_direct = 0
    tile_prefix reads the sums of a full block of 1,024 tiles, of full blocks of 32 (one of them
    without a line end) and of single tiles; ingest_tiles = 3 ranges pass every block seam."""
    _check_coarse(W.COARSE_TILES, ({}, {"ingest_direct": 0}, {"ingest_tiles": 3}, {"ingest_direct": 0, "ingest_tiles": 3}))


def test_whitelist_past_the_resident_grid():
    """Piece (b), 8 tiles per compute unit and 3 more (8 workgroups of 256 threads is the most a
    compute unit holds): wl_count_kernel's workgroups take a second tile, and the encode pass's
    default range -- one per resident slot -- is more than one tile (three at the encode kernel's
    three workgroups per compute unit)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ntiles = cus * 8 + 3
    # the range the library takes is ceil(ntiles / min(ntiles, cus * w)), w workgroups per compute unit
    print("piece (b): %d compute units, %d tiles; default per_wg by resident workgroups per compute unit: %s"
          % (cus, ntiles, {w: -(-ntiles // (cus * w)) for w in range(1, 9)}))
    assert all(-(-ntiles // (cus * w)) >= 2 for w in range(1, 9))
    _check_coarse(ntiles, ({},))


# ---------------------------------------------------------------- sct_lines
def _lines_call(d_buf, nbytes, cap, rows):
    import torch
    from sctools_amd import _lib
    starts = torch.full((rows,), FILL["starts"], dtype=torch.int64, device="cuda")
    lens = torch.full((rows,), FILL["lens"], dtype=torch.int32, device="cuda")
    nl, mx = ctypes.c_int64(-1), ctypes.c_int32(-1)
    _lib.check(_lib.lib().sct_lines(d_buf.data_ptr(), nbytes, cap, starts.data_ptr(), lens.data_ptr(),
                                    ctypes.byref(nl), ctypes.byref(mx), None))
    return nl.value, mx.value, starts.cpu().numpy(), lens.cpu().numpy()


def _check_lines(data, ref, what, d_buf=None):
    """A sizing call, a capacity one below the count (nothing filled, longest line 0), room for all."""
    d_buf = _upload(data) if d_buf is None else d_buf
    rows = ref.n + GUARD
    for cap in (0, ref.n - 1, ref.n, rows):
        n, mx, starts, lens = _lines_call(d_buf, len(data), cap, rows)
        filled = cap >= ref.n and cap > 0
        assert (n, mx) == (ref.n, ref.maxlen if filled else 0), (what, "capacity %d: lines, longest line" % cap, (n, mx))
        m = ref.n if filled else 0
        assert np.array_equal(starts[:m], ref.starts[:m]), "%s: capacity %d: starts: %s" % (what, cap, _first_bad(starts[:m], ref.starts[:m]))
        assert np.array_equal(lens[:m], ref.lens[:m]), "%s: capacity %d: lens: %s" % (what, cap, _first_bad(lens[:m], ref.lens[:m]))
        assert (starts[m:] == FILL["starts"]).all() and (lens[m:] == FILL["lens"]).all(), \
            (what, "capacity %d: a row past the lines was written" % cap)


@pytest.mark.parametrize("family", sorted(W.FAMILIES) + [W.GC_FAMILY])
def test_lines_seams(family):
    """sct_lines (line_count_kernel, the scan, line_starts_kernel, line_lens_kernel) on every small
    case: 4 KiB tiles, so 20 and more tile offsets from the scan."""
    for i, c in enumerate(W.cases(family)):
        if family == "cap" and i % 3:
            continue  # (the same bytes three times)
        _check_lines(c.data, _lines(family, i), c.desc)


def test_lines_past_blocks_of_tiles_and_the_length_grid():
    """Piece (a): 4,232 tiles of 4 KiB, most of them without a line end; and 600,000 empty lines:
    more lines than line_lens_kernel's grid of 2,048 workgroups has threads."""
    data = W.coarse_piece(W.COARSE_TILES)
    _check_lines(data, W.read_lines(data), "%d tiles" % W.COARSE_TILES)
    n = W.EMPTY_LINES
    ref = W.Lines(n, 0, np.arange(n, dtype=np.int64), np.zeros(n, np.int32))
    small = W.read_lines(b"\n" * 1000)
    assert small.n == 1000 and np.array_equal(small.starts, np.arange(1000)) and not small.lens.any()
    _check_lines(b"\n" * n, ref, "%d empty lines" % n)
    # the same with a longest line that only a thread's second step sees
    data = b"\n" * (n - 2) + b"ACGTACG\n"
    ref = W.Lines(n - 1, 7, np.arange(n - 1, dtype=np.int64), np.array([0] * (n - 2) + [7], np.int32))
    _check_lines(data, ref, "%d empty lines and one of 7 bases" % (n - 2))


# ---------------------------------------------------------------- the host forms
def test_whitelist_encode_host_call_in_ranges_of_two_tiles():
    """_lib.whitelist_encode (the sizing call, then the filling call through the host stage) with
    two tiles per workgroup, on two ragged cases."""
    from sctools_amd import _lib
    for family, i in (("lf", 17), ("split", 100)):
        c, ref = W.cases(family)[i], _lines(family, i)
        for kind in (2, 3):
            words = _lib.words_for_bits(kind * ref.maxlen)
            enc = _enc(family, i, kind, words)
            with _lib.tuning(ingest_tiles=2):
                codes, starts, lens, flags = _lib.whitelist_encode(c.data, kind)
            assert codes.shape == (ref.n, words) and words == 2
            for name, a, b in (("codes", codes, enc.codes), ("starts", starts, ref.starts), ("lens", lens, ref.lens),
                               ("flags", flags, enc.flags)):
                assert np.array_equal(a, b), "%s [kind %d]: %s: %s" % (c.desc, kind, name, _first_bad(a, b))


def test_from_whitelist_in_ranges_of_two_tiles(tmp_path):
    """Barcodes.from_whitelist on a fixed-stride file, two tiles per workgroup: the Counter of the
    oracle's codes of every line[:-1], in file order."""
    from sctools_amd import _lib, barcode
    (c,) = [c for c in W.cases("fixed") if not W.claim(c, "flag_line")]
    p = tmp_path / "whitelist.txt"
    p.write_bytes(c.data)
    with open(p, "rb") as f:
        want = Counter(O.two_bit_encode(line[:-1]) for line in f)
    with _lib.tuning(ingest_tiles=2):
        got = barcode.Barcodes.from_whitelist(str(p), 12)
    assert list(got) == list(want) and [got[k] for k in got] == list(want.values())
    assert len(want) > 500 and max(want.values()) > 1 and sum(want.values()) == W.FIXED_BYTES // 13
