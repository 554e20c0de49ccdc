"""GPU: every path of the record encoders (the kernels of sctools_amd/csrc/encode.hip, the host
stream and array calls of encode_host.cpp) byte for byte against tests/encode_reference.py, on
inputs that carry all 256 byte values at every position; and the limb seams of the decode, gc and
hamming kernels against the oracle on Python ints.  Exact integer equality on every record: nothing
is sampled and nothing has a tolerance."""

import ctypes
import random

import numpy as np
import pytest

import encode_reference as R
from oracle import oracle as O
from sctools_amd import _lib, encodings

pytestmark = pytest.mark.gpu

TwoBit, ThreeBit = encodings.TwoBit, encodings.ThreeBit
GUARD = 64
CODE_SENTINEL = 0x5A5A5A5A5A5A5A5A
BYTE_SENTINEL = 0xA5


def _same(got, want, what):
    """Exact equality of (codes, gc, flags) on every record; names the first record that differs."""
    for name, g, w in zip(("codes", "gc", "flags"), got, want):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        if name == "codes":
            g, w = g.reshape(len(g), -1), w.reshape(len(w), -1)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
            r = int(bad[0])
            raise AssertionError("%s: %s differ in %d records, first %d: got %s want %s"
                                 % (what, name, bad.size, r, g[r].tolist(), w[r].tolist()))


def _host_encode(kind, recs):
    return _lib.encode(kind, recs, recs.shape[1])


# ---------------------------------------------------------------- a. the tiled kernel, default grid
def _tiled_n(L):
    return max(2 * 256 * L, 2048) + 1024 + 37


TILED_CASES = ([(2, L) for L in (4, 8, 12, 16, 20, 24, 28, 32)]      # TwoBit fast path
               + [(2, L) for L in (1, 2, 3, 5, 15, 17, 31)]          # TwoBit byte loop, staging tail
               + [(3, L) for L in (4, 8, 16, 20)]                    # ThreeBit dword LUT
               + [(3, L) for L in (1, 7, 15, 21)])                   # ThreeBit byte loop


@pytest.mark.parametrize("kind,L", TILED_CASES)
def test_tiled_default_grid(kind, L):
    n = _tiled_n(L)
    recs = R.records(n, L, seed=1000 * kind + L)
    R.check_input(recs, full=True)
    if L % 4:
        assert n * L % 16  # the last tile's bytes beyond its 16-byte loads are staged one by one
    _same(_host_encode(kind, recs), R.encode(kind, recs), "kind %d L %d n %d" % (kind, L, n))


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("L", [16, 15])
def test_tiled_dispatch_threshold(kind, L):
    """n on both sides of the first and the second tile boundary.  One batch is too small to hold
    every (value, position) pair, so the six batches walk the table between them."""
    batches, phase = [], 0
    total = np.zeros((L, 256), bool)
    for n in (1023, 1024, 1025, 2047, 2048, 2049):
        recs = R.records(n, L, seed=n + kind, phase=phase)
        total |= R.check_input(recs, phase=phase)
        batches.append(recs)
        phase += n // 2
    R.assert_covered(total)
    for recs in batches:
        _same(_host_encode(kind, recs), R.encode(kind, recs), "kind %d L %d n %d" % (kind, L, len(recs)))


# ---------------------------------------------------------------- device-pointer calls
def _device_encode(kind, data, offset, n, stride, L, want_gc=True, want_flags=True):
    """sct_encode on device pointers: records at (a 256-aligned pointer + offset) + r * stride in
    `data`; every output lies between GUARD rows of a sentinel on either side, checked here."""
    import torch
    dev = torch.device("cuda", 0)
    words = R.words_for(kind, L)
    assert data.size >= (n - 1) * stride + L
    d_in = torch.empty(offset + data.size + 16, dtype=torch.uint8, device=dev)
    assert d_in.data_ptr() % 256 == 0
    d_in[offset:offset + data.size] = torch.from_numpy(data).to(dev)
    rows = n + 2 * GUARD
    codes = torch.full((rows, words), CODE_SENTINEL, dtype=torch.int64, device=dev)
    gc = torch.full((rows,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    flags = torch.full((rows,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().sct_encode(kind, d_in.data_ptr() + offset, n, stride, L,
                                     codes.data_ptr() + GUARD * words * 8,
                                     gc.data_ptr() + GUARD if want_gc else None,
                                     flags.data_ptr() + GUARD if want_flags else None, None))
    torch.cuda.synchronize()
    c = codes.cpu().numpy().view(np.uint64)
    g, f = gc.cpu().numpy(), flags.cpu().numpy()
    for arr, s in ((c, CODE_SENTINEL), (g, BYTE_SENTINEL), (f, BYTE_SENTINEL)):
        assert (arr[:GUARD] == s).all() and (arr[GUARD + n:] == s).all(), "guard rows overwritten"
    if not want_gc:
        assert (g == BYTE_SENTINEL).all()
    if not want_flags:
        assert (f == BYTE_SENTINEL).all()
    return c[GUARD:GUARD + n], g[GUARD:GUARD + n] if want_gc else None, f[GUARD:GUARD + n] if want_flags else None


def _strided(recs, stride, seed):
    """The records `stride` bytes apart, bytes of neither TwoBit map between and after them."""
    n, L = recs.shape
    rng = np.random.default_rng(seed)
    rows = R.GARBAGE[rng.integers(0, len(R.GARBAGE), (n, stride))]
    rows[:, :L] = recs
    return np.ascontiguousarray(rows.reshape(-1))


# ---------------------------------------------------------------- b. the resident grid
@pytest.mark.parametrize("kind,L", [(2, 4), (2, 32), (2, 15), (3, 20), (3, 21)])
def test_tiled_resident_grid(kind, L):
    """SCT_TUNE_ENCODE_GRID = 0: as many workgroups as are resident, each looping over tiles with
    the next tile's loads in flight.  A compute unit holds at most 32 waves = 8 workgroups of 256,
    so 8 CUs + 3 full tiles and a ragged one exceed any resident grid: some workgroups run two or
    three tiles."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus + 3) * 1024 + 517
    recs = R.records(n, L, seed=77 * kind + L)
    R.check_input(recs, full=True)
    want = R.encode(kind, recs)
    with _lib.tuning(encode_grid=0):
        got = _device_encode(kind, recs.reshape(-1), 0, n, L, L)
    _same(got, want, "resident kind %d L %d n %d" % (kind, L, n))


# ---------------------------------------------------------------- c. sct_encode: strides and alignments
OFFSETS = (0, 1, 2, 3, 4, 8, 16)


def _strides(L):
    return (L, L + 1, L + 4, 2 * L + 3)


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("L", [1, 4, 16, 28, 33, 43, 64, 100])
def test_device_pointer_strides_and_alignments(kind, L):
    """Every (pointer offset, stride): the dword reader (L, stride and pointer all multiples of
    4), the byte reader, one and several limbs (L = 43 at 3 bits: a triplet straddles limbs 1 and
    2).  n = 1000 stays in encode_kernel; at n = 5000 the 16-byte-aligned, stride == L, one-limb
    calls take the tiled kernel."""
    combos = [(off, st) for off in OFFSETS for st in _strides(L)]
    # One batch is too small for the whole (value, position) table, so the batches walk it: a fresh
    # window for every n = 1000 call, then one for the n = 5000 calls of every pointer offset
    # (28 * 500 + 7 * 2500 = 31,500 first replacements; L = 100 needs 25,600).
    n, phase = 1000, 0
    small, big, want_big = [], {}, {}
    total = np.zeros((L, 256), bool)
    for k in range(len(combos)):
        recs = R.records(n, L, seed=31 * L + k, phase=phase)
        total |= R.check_input(recs, phase=phase, full=False)
        small.append(recs)
        phase += n // 2
    for off in OFFSETS:
        big[off] = R.records(5000, L, seed=7 * L + kind + off, phase=phase)
        total |= R.check_input(big[off], phase=phase, full=False)
        want_big[off] = R.encode(kind, big[off])
        phase += 2500
    R.assert_covered(total)
    for k, (off, st) in enumerate(combos):
        got = _device_encode(kind, _strided(small[k], st, k), off, n, st, L)
        _same(got, R.encode(kind, small[k]), "kind %d L %d n %d offset %d stride %d" % (kind, L, n, off, st))
        got = _device_encode(kind, _strided(big[off], st, k), off, 5000, st, L)
        _same(got, want_big[off], "kind %d L %d n 5000 offset %d stride %d" % (kind, L, off, st))


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("n,L,stride", [(5000, 16, 16), (1000, 33, 36)])
def test_device_pointer_optional_outputs(kind, n, L, stride):
    # one batch: its window starts at the last position and wraps to the first, so the cycled bytes
    # lie in the last dword and the lowest bits, and in the first dword and the top limb
    phase = 256 * (L - 1)
    recs = R.records(n, L, seed=n + L, phase=phase)
    seen = R.check_input(recs, phase=phase, full=False)
    assert seen[L - 1].all() and seen[0].any()
    want = R.encode(kind, recs)
    data = _strided(recs, stride, 3)
    _same(_device_encode(kind, data, 0, n, stride, L, want_gc=False), want, "gc = NULL")
    _same(_device_encode(kind, data, 0, n, stride, L, want_flags=False), want, "flags = NULL")


# ---------------------------------------------------------------- d. sct_encode_var, one limb
def _var_input(kind, seed, reps=192):
    """Records of every length 0..maxL at every start offset mod 4, `reps` times each in a shuffled
    order, bytes of neither TwoBit map between them; the byte-cycling replacements in every second
    record.  The buffer's length is a multiple of 4 with at least 4 bytes after the last record."""
    maxL = 32 if kind == 2 else 21
    rng = np.random.default_rng(seed)
    pairs = np.array([(o, L) for L in range(maxL + 1) for o in range(4)] * reps)
    pairs = pairs[rng.permutation(len(pairs))]
    n = len(pairs)
    starts = np.zeros(n, np.int64)
    end = 0
    for i, (o, L) in enumerate(pairs.tolist()):
        starts[i] = end + 1 + (o - (end + 1)) % 4  # at least one byte between two records
        end = starts[i] + L
    size = (end + 4 + 3) // 4 * 4
    buf = R.GARBAGE[rng.integers(0, len(R.GARBAGE), size)]
    lens = pairs[:, 1].astype(np.int32)
    lane_seen = np.zeros((4, 256), bool)  # byte lane of the aligned dword the replacement lies in
    pos_seen = np.zeros((4, 256), bool)   # its position in the record, mod 4
    ndw = (3 + maxL - 1) // 4 + 1         # aligned dwords a record can span: 9 at 32 bytes
    dword_flag = np.zeros((ndw, 3), np.int64)  # dword k of a record's window holding a base / ambiguous / other byte
    for i in range(n):
        L = int(lens[i])
        rec = R.BASES[rng.integers(0, 8, L)]
        if L and i % 2:
            for pos, val in R.substitutions(i, L):
                rec[pos] = val
            lane_seen[(starts[i] + pos) % 4, val] = True
            pos_seen[pos % 4, val] = True
            np.add.at(dword_flag, ((starts[i] % 4 + np.arange(L)) // 4, R.F2[rec]), 1)
        buf[starts[i]:starts[i] + L] = rec
    # the conditions on this input
    assert size % 4 == 0 and size - end >= 4
    count = np.zeros((4, maxL + 1), np.int64)
    np.add.at(count, (starts % 4, lens), 1)
    assert count.min() >= 64
    assert lane_seen.all() and pos_seen.all()
    assert (dword_flag > 0).all()  # every dword of the realigned window meets a byte of each class
    return buf, starts, lens


@pytest.mark.parametrize("kind", [2, 3])
def test_encode_var_one_limb_every_record(kind):
    """encode_var_kernel: the realigned dword reads at every (start offset mod 4, length), with the
    code and gc of flagged records compared too."""
    import torch
    buf, starts, lens = _var_input(kind, seed=40 + kind)
    n = starts.size
    want = R.encode_var(kind, buf, starts, lens)
    assert (want[2] == 0).any()
    if kind == 2:
        assert (want[2] == 1).any() and (want[2] == 2).any()
    dev = torch.device("cuda", 0)
    d_buf = torch.from_numpy(buf).to(dev)
    assert d_buf.data_ptr() % 4 == 0
    d_st, d_len = torch.from_numpy(starts).to(dev), torch.from_numpy(lens).to(dev)
    rows = n + 2 * GUARD
    codes = torch.full((rows,), CODE_SENTINEL, dtype=torch.int64, device=dev)
    gc = torch.full((rows,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    flags = torch.full((rows,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().sct_encode_var(kind, d_buf.data_ptr(), d_st.data_ptr(), d_len.data_ptr(), n, 1,
                                         codes.data_ptr() + 8 * GUARD, gc.data_ptr() + GUARD,
                                         flags.data_ptr() + GUARD, None))
    torch.cuda.synchronize()
    c, g, f = codes.cpu().numpy().view(np.uint64), gc.cpu().numpy(), flags.cpu().numpy()
    for arr, s in ((c, CODE_SENTINEL), (g, BYTE_SENTINEL), (f, BYTE_SENTINEL)):
        assert (arr[:GUARD] == s).all() and (arr[GUARD + n:] == s).all(), "guard rows overwritten"
    _same((c[GUARD:GUARD + n], g[GUARD:GUARD + n], f[GUARD:GUARD + n]), want, "encode_var kind %d" % kind)


# ---------------------------------------------------------------- e. the host stream
@pytest.mark.parametrize("kind,L", [(2, 16), (2, 15), (3, 21)])
def test_encode_stream_every_record(kind, L):
    """Three chunks (the stream's floor is 2^18 records a chunk), the last one ragged."""
    n = 600_011
    recs = R.records(n, L, seed=600 + L)
    R.check_input(recs, full=True)
    want = R.encode(kind, recs)
    codes, gc, flags = _lib.encode_stream(kind, recs, chunk=1 << 18)
    _same((codes, gc, flags), want, "stream kind %d L %d" % (kind, L))


def _guarded_host(n, dtype, sentinel, page_locked):
    """n + 2 GUARD rows of the sentinel in host memory, page-locked (the library's pool) or pageable."""
    rows = n + 2 * GUARD
    a = _lib.pinned.empty(rows, dtype) if page_locked else np.empty(rows, dtype)
    assert _lib.host_pinned(a) == page_locked
    a[:] = sentinel
    return a


def _stream_into(kind, src, n, L, outs, chunk):
    """sct_encode_stream_host itself, the outputs GUARD rows into `outs` (codes, gc, flags)."""
    at = [ctypes.c_void_p(a.ctypes.data + GUARD * a.itemsize) for a in outs]
    return _lib.lib().sct_encode_stream_host(kind, _lib._ptr(src), n, L, at[0], at[1], at[2], chunk)


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("L", [5, 16])
def test_encode_stream_mixed_outputs(kind, L):
    """Page-locked and pageable arrays in one call: each array is copied in place or through the
    stage on its own.  Five chunks of 2^18 records, so stages 0 and 1 are each used twice; the last
    chunk's 37 records are fewer than a tile and take encode_kernel.  L = 5: the tiled kernel's byte
    path and staging tail."""
    n = 4 * (1 << 18) + 37
    recs = R.records(n, L, seed=900 + 10 * kind + L)
    R.check_input(recs, full=True)
    want = R.encode(kind, recs)
    pin_in = _lib.pinned.empty((n, L), np.uint8)
    pin_in[:] = recs
    assert _lib.host_pinned(pin_in) and not _lib.host_pinned(recs)
    for codes_locked in (True, False):
        for src in (pin_in, recs):
            outs = (_guarded_host(n, np.uint64, CODE_SENTINEL, codes_locked),
                    _guarded_host(n, np.uint8, BYTE_SENTINEL, not codes_locked),
                    _guarded_host(n, np.uint8, BYTE_SENTINEL, not codes_locked))
            _lib.check(_stream_into(kind, src, n, L, outs, 1 << 18))
            for a, s in zip(outs, (CODE_SENTINEL, BYTE_SENTINEL, BYTE_SENTINEL)):
                assert (a[:GUARD] == s).all() and (a[GUARD + n:] == s).all(), "guard rows overwritten"
            _same(tuple(a[GUARD:GUARD + n] for a in outs), want,
                  "stream kind %d L %d codes %s input %s" % (kind, L, "page-locked" if codes_locked else "pageable",
                                                            "page-locked" if src is pin_in else "pageable"))


def test_encode_stream_one_chunk_and_none():
    kind, L = 2, 16
    n = (1 << 18) + 1
    recs = R.records(n, L, seed=262)
    R.check_input(recs, full=True)
    want = R.encode(kind, recs)
    # chunk = 0: the floor of 2^18 records a chunk, so a full chunk and one of a single record
    _same(_lib.encode_stream(kind, recs, chunk=0), want, "stream n 2^18 + 1")
    _same(_lib.encode_stream(kind, recs[:1]), tuple(w[:1] for w in want), "stream n 1")
    outs = (_guarded_host(0, np.uint64, CODE_SENTINEL, False), _guarded_host(0, np.uint8, BYTE_SENTINEL, False),
            _guarded_host(0, np.uint8, BYTE_SENTINEL, False))
    assert _stream_into(kind, recs, 0, L, outs, 0) == _lib.SCT_OK
    for a, s in zip(outs, (CODE_SENTINEL, BYTE_SENTINEL, BYTE_SENTINEL)):
        assert (a == s).all(), "n = 0 wrote something"


# ---------------------------------------------------------------- f. the drop-in, end to end
def _iupac_batch(L, seed):
    rng = np.random.default_rng(seed)
    recs = R.BASES[rng.integers(0, 8, (3000, L))]
    amb = rng.random(recs.shape) < 0.03
    recs[amb] = R.IUPAC[rng.integers(0, len(R.IUPAC), int(amb.sum()))]
    flags = R.encode(2, recs)[2]
    assert (flags == 0).any() and (flags == 1).any() and not (flags & 2).any()
    return recs


@pytest.mark.parametrize("L", [16, 15])
def test_dropin_two_bit_encode_array_with_iupac(L):
    """TwoBit.encode_array ORs its draws into the bits the kernel left at ambiguous positions: the
    codes and the generator's state afterwards equal the oracle's per-record loop."""
    recs = _iupac_batch(L, seed=L)
    random.seed(1234 + L)
    want = [O.two_bit_encode(r.tobytes()) for r in recs]
    state = random.getstate()
    random.seed(1234 + L)
    got = TwoBit.encode_array(recs)
    assert random.getstate() == state
    assert got.tolist() == want


@pytest.mark.parametrize("L", [16, 15])
def test_dropin_two_bit_encode_array_invalid_byte(L):
    recs = _iupac_batch(L, seed=L)
    recs[2500, L // 2] = ord("#")
    assert R.encode(2, recs[2500:2501])[2][0] & 2
    random.seed(99 + L)
    with pytest.raises(KeyError) as want:
        for r in recs:
            O.two_bit_encode(r.tobytes())
    state = random.getstate()
    random.seed(99 + L)
    with pytest.raises(KeyError) as got:
        TwoBit.encode_array(recs)
    assert got.value.args == want.value.args
    assert random.getstate() == state


@pytest.mark.parametrize("L", [16, 15, 21])
def test_dropin_three_bit_encode_array_arbitrary_bytes(L):
    rng = np.random.default_rng(300 + L)
    recs = rng.integers(0, 256, (3000, L), dtype=np.uint8)
    recs[::3] = R.BASES[rng.integers(0, 8, (1000, L))]
    got, gc = ThreeBit.encode_array(recs, return_gc=True)
    want = [O.three_bit_encode(r.tobytes()) for r in recs]
    assert got.tolist() == want
    assert gc.tolist() == [O.three_bit_gc(w) for w in want]


# ---------------------------------------------------------------- g. limb seams of the other record kernels
def _random_ints(rng, count, bits):
    return [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(count)]


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("words", [2, 3])
def test_hamming_across_limbs(kind, words):
    """b = a ^ (m << p) for every bit offset p: a difference of one to three bits anywhere, the
    groups that straddle two limbs included."""
    rng = np.random.default_rng(10 * kind + words)
    bits = 64 * words
    a, b = [], []
    for x in [0] + _random_ints(rng, 3, bits):
        for p in range(bits - 2):
            for m in range(1, 8 if kind == 3 else 4):
                a.append(x)
                b.append(x ^ (m << p))
    assert max(v.bit_length() for v in b) <= bits
    la, lb = _lib.ints_to_limbs(a, words), _lib.ints_to_limbs(b, words)
    enc, ref = (TwoBit, O.two_bit_hamming) if kind == 2 else (ThreeBit, O.three_bit_hamming)
    got = enc.hamming_distance_array(la, lb)
    assert got.tolist() == [ref(x, y) for x, y in zip(a, b)]


@pytest.mark.parametrize("words", [2, 3])
def test_gc_across_limbs(words):
    rng = np.random.default_rng(20 + words)
    bits = 64 * words
    codes = [1 << p for p in range(bits)] + _random_ints(rng, 200, bits)
    limbs = _lib.ints_to_limbs(codes, words)
    for L in (32, 33, 63, 64, 65, 96):  # the code's bits above 2 L are not read
        got = TwoBit(L).gc_content_array(limbs)
        assert got.tolist() == [O.two_bit_gc(c, L) for c in codes], L
    got = ThreeBit.gc_content_array(limbs)
    assert got.tolist() == [O.three_bit_gc(c) for c in codes]


@pytest.mark.parametrize("L", [21, 22, 42, 43, 63, 64])
def test_decode3_across_limbs(L):
    """Triplets 21 and 42 straddle limbs 0 / 1 and 1 / 2.  A triplet of 0, 5 or 7 raises the
    reference's KeyError (a 0 in the top triplet only shortens the sequence)."""
    rng = np.random.default_rng(L)
    words = max(2, -(-3 * L // 64))
    seqs = [bytes(rng.choice(list(b"ACGTN"), L).tolist()) for _ in range(200)]
    codes = [O.three_bit_encode(s) for s in seqs]
    assert [O.three_bit_decode(c) for c in codes] == seqs
    assert ThreeBit.decode_array(_lib.ints_to_limbs(codes, words)) == seqs
    bad = []
    for c in codes[:3]:
        for t in range(L):
            for v in (0, 5, 7):
                bad.append(c & ~(7 << (3 * t)) | (v << (3 * t)))
    want = []
    for c in bad:
        try:
            want.append(O.three_bit_decode(c))
        except KeyError as e:
            want.append(e.args)
    assert sum(isinstance(w, tuple) for w in want) == len(bad) - 3  # all but the three top-triplet zeros
    limbs = _lib.ints_to_limbs(bad, words)
    out, lengths, err = _lib.decode3(limbs)
    got = [(int(err[r]),) if err[r] >= 0 else out[r, out.shape[1] - lengths[r]:].tobytes() for r in range(len(bad))]
    assert got == want
    with pytest.raises(KeyError) as ei:  # the drop-in raises at the first such record
        ThreeBit.decode_array(limbs)
    assert ei.value.args == next(w for w in want if isinstance(w, tuple))


@pytest.mark.parametrize("words", [2, 3])
@pytest.mark.parametrize("L", [32, 33, 64, 65, 96])
def test_decode2_across_limbs(words, L):
    rng = np.random.default_rng(100 * words + L)
    codes = _random_ints(rng, 300, 64 * words) + [0, (1 << (64 * words)) - 1]
    got = TwoBit(L).decode_array(_lib.ints_to_limbs(codes, words))
    assert [bytes(x) for x in got] == [O.two_bit_decode(c, L) for c in codes]
