"""Every SPECTRAL seed form against the formula (tests/seed_reference.py), exact to the byte, through
sct_allpairs_seed_rows: the rows the tile reads, written by the kernel and grid count() launches for
the range.  The tile squares the transform and sums whole weight classes, so a permuted or negated
row changes no histogram: the bytes are the check.

  forms   i16   int16 seeds on 14-bit columns (seed_body<int16_t>: two slices per staged dword)
          i32   int32 seeds on 14-bit columns (seed_body<int32_t>)
          c16   int8 seeds on 16-bit columns (seed16_sm_kernel: 16 planes, 2^16 slices)
          i8    int8 seeds on 14-bit columns (seed_sm_kernel), where test_gpu_seed_bytes.py stops:
                lanes permuted by group count, and the Gray-ordered walk blocks
          int16 / int32 rows hold column c at seed_reference.row_position(c)
  small   whole ranges, every byte: ranges that start and end inside a walk, odd ends (the int16
          seed's slice pairs), the first and the last slice alone; at most ~330 slices where a row is
          64 KiB
  shapes  the launch shapes of a whole job, one launch each, sampled rows: Gray blocks of 2 and of
          16 walks (int8 seeds: a walk starts from the previous one's last state, walks outside
          the range are skipped "as if walked") and two strided walks per workgroup (int16 / int32
          seeds: the LDS stage reused).  The sample holds the partial first and last block, two
          whole interior blocks and one slice of every walk.
  rule    what the call refuses, writing nothing

Buffers hold 0x55 before the call and one row more than the range: the tail must still hold it.
An element of a wide seed cannot equal the fill (asserted on the reference: |seed| < 0x5555 for
int16; an int32 element would have to be 0x55555555), nor can a whole int8 row.
A shapes case takes under a second on an MI355X, launch, gather, reference and compare together
(the two 1 GiB cases 0.65 s and 0.80 s, the others 0.25 s at most); the whole file 17 s."""
import functools

import numpy as np
import pytest

import seed_reference as R
from sctools_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

FILL = 0x55
FILL_ELEM = {1: 0x55, 2: 0x5555, 4: 0x55555555}
FORMS = {"i16": (14, 2), "i32": (14, 4), "c16": (16, 1), "i8": (14, 1)}  # (column_bits, elem_bytes)
# the wide seeds only exist on forced 14-bit columns here: their sets' 16-bit columns hold <= 127 codes
KNOBS = {"i16": {"spectral_columns": 14}, "i32": {"spectral_columns": 14}, "c16": {"spectral_columns": 16}, "i8": {}}
Z0 = 64 * 53 + 17  # neither walk- nor block-aligned


def _column(col, count, seed, column_bits=14, same=0):
    """`count` distinct codes in column `col`, then `same` copies of one more."""
    hi = np.random.default_rng(seed).choice(1 << (32 - column_bits), count + (same > 0), replace=False).astype(np.uint64)
    hi = np.concatenate([hi[:count], np.repeat(hi[count:], same)])
    return (hi << np.uint64(column_bits)) | np.uint64(col)


def _sparse(n, seed):
    return synthetic.whitelist_codes(n, 16, seed=seed)


SETS = {
    # dense 14-bit columns that differ in bits 3, 12 and 13 (row_position moves bit 3), in the first
    # (0x00xx) and the last (0x3Fxx) 256-column block, over 3,000 sparse codes
    "i16": ["c128", "c200", "same300", "c97_65"],
    "i32": ["c33000"],
    "c16": ["sparse3000", "col127", "cols64_65", "dense5003", "groups1234"],
    "i8": ["groups1234"],
}


def _groups1234(block, column_bits):
    """columns of 1, 33, 65 and 97 codes (1-4 groups) out of column order inside one 256-column
    block, so seed_lane_column's three classes all move lanes"""
    sizes = {0x05: 1, 0x42: 97, 0x43: 33, 0x81: 65, 0xC7: 1, 0xC8: 97, 0xFE: 33, 0xFF: 65}
    return [_column(block | o, m, 60 + i, column_bits) for i, (o, m) in enumerate(sorted(sizes.items()))]


@functools.lru_cache(maxsize=None)
def codes_of(form, name):
    if form == "i16":
        parts = [_sparse(3000, 11), _column(0x0003, 40, 41), _column(0x3FFC, 50, 42)]
        if name == "c128":  # the smallest int16 plan
            parts.append(_column(0x0008, 128, 43))
        elif name == "c200":
            parts.append(_column(0x1AA0, 200, 44))
        elif name == "same300":  # seed +-300: negative low halves beside positive high halves in a dword
            parts.append(_column(0x2AA8, 0, 45, same=300))
        elif name == "c97_65":  # four and three groups beside each other: planes past the two in registers
            parts += [_column(0x3FF7, 97, 46), _column(0x3FF8, 65, 47), _column(0x1AA0, 200, 44)]
        else:
            raise KeyError(name)
        return np.concatenate(parts)
    if form == "i32":  # 32,000 distinct codes and 1,000 copies of one more in a column, 3,000 sparse
        return np.concatenate([_sparse(3000, 11), _column(0x2B5C, 32000, 51, same=1000)])
    if form == "i8":
        return np.concatenate([_sparse(1000, 13)] + _groups1234(0x3F00, 14))
    if name == "sparse3000":
        return _sparse(3000, 11)
    if name == "col127":  # one column of 127 codes alone: four groups, the int8 limit
        return _column(0xAB5C, 127, 21, 16)
    if name == "cols64_65":  # neighbours: two groups exactly full, one code in the third
        return np.concatenate([_column(0x1234, 64, 22, 16), _column(0x1235, 65, 23, 16)])
    if name == "dense5003":  # 5,003 random codes and 100 more in a column of the last block
        return np.unique(np.concatenate([_sparse(5003, 12), _column(0xFFF7, 100, 24, 16)]))
    if name == "groups1234":
        return np.concatenate([_sparse(1000, 13)] + _groups1234(0xFF00, 16))
    raise KeyError(name)


def dense5003_14():
    """test_gpu_seed_bytes.py's dense set"""
    return np.unique(np.concatenate([_sparse(5003, 12), _column(0x3FF7, 100, 24)]))


def ranges(column_bits, cap):
    """test_gpu_seed_bytes.RANGES on 2^(32 - column_bits) slices, a range cut to `cap` slices"""
    S = 1 << (32 - column_bits)
    return [(0, 1), (0, 256), (255, 257), (777, min(2277, 777 + cap)), (1000, min(3600, 1000 + cap)), (S - 1, S)]


class Plan:
    """a built plan of the intended form, its codes kept alive"""

    def __init__(self, torch, form, codes):
        self.torch, self.form = torch, form
        self.column_bits, self.elem_bytes = FORMS[form]
        self.row_bytes = (1 << self.column_bits) * self.elem_bytes
        self.d_codes = torch.from_numpy(codes.view(np.int64)).cuda()
        with _lib.tuning(spectral_chunk=4096, **KNOBS[form]):
            self.plan = _lib.AllPairsPlan(self.d_codes.data_ptr(), codes.size, 32, scheme=_lib.SCHEME_SPECTRAL)
        try:
            info = self.plan.spectral_info()
            assert (info["column_bits"], info["elem_bytes"]) == FORMS[form], info
            self.plan.build()
        except BaseException:
            self.plan.close()
            raise

    def rows(self, z0, z1):
        """[z1 - z0 + 1][row bytes] uint8 on the device: the range's rows and a tail row of fill"""
        n = z1 - z0
        buf = self.torch.full((n + 1, self.row_bytes), FILL, dtype=self.torch.uint8, device="cuda")
        self.plan.seed_rows(buf.data_ptr(), n * self.row_bytes, z0, z1)
        self.torch.cuda.synchronize()
        return buf

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.plan.close()


def check_reference(ref, elem_bytes):
    """the fill cannot pass for written values"""
    if elem_bytes == 1:
        assert not (ref == FILL).all(axis=1).any()
    else:  # int16: |seed| < 0x5555; int32 (a column of 33,000 codes reaches 33,000): < 0x55555555
        assert np.abs(ref).max() < FILL_ELEM[elem_bytes]


def differing(got, want, slices, elem_bytes):
    """the first eight (slice, column, got, want) that differ"""
    bad = np.argwhere(got != want)
    column = np.arange(got.shape[1])
    if elem_bytes > 1:
        column = np.empty(1 << 14, np.int64)
        column[R.row_position(np.arange(1 << 14), elem_bytes)] = np.arange(1 << 14)
    return len(bad), [(int(slices[r]), int(column[p]), int(got[r, p]), int(want[r, p])) for r, p in bad[:8]]


def host_rows(dev_rows, elem_bytes):
    return dev_rows.cpu().numpy().view(R.DTYPES[elem_bytes])


SMALL = [(form, name, rng) for form in FORMS for name in SETS[form] for rng in range(6)]


@pytest.mark.parametrize("form,name,rng", SMALL, ids=["%s-%s-r%d" % c for c in SMALL])
def test_small_ranges_every_byte(form, name, rng):
    torch = pytest.importorskip("torch")
    column_bits, elem_bytes = FORMS[form]
    z0, z1 = ranges(column_bits, 2600 if form in ("i16", "i8") else 330)[rng]
    codes = codes_of(form, name)
    ref = R.rows(codes, column_bits, z0, z1)
    check_reference(ref, elem_bytes)
    want = R.stored(ref, column_bits, elem_bytes)
    with Plan(torch, form, codes) as p:
        buf = p.rows(z0, z1)
    assert bool((buf[z1 - z0] == FILL).all()), "bytes after the range were written"
    got = host_rows(buf[:z1 - z0], elem_bytes)
    nbad, first = differing(got, want, np.arange(z0, z1), elem_bytes)
    print("%s %s [%d, %d): %d values, %d differ from the formula" % (form, name, z0, z1, want.size, nbad))
    assert nbad == 0, first


def sample(z0, z1, lp, interior):
    """Slices of [z0, z1): all of the first and the last block of 2^lp walks the range touches, all
    of the blocks `interior`, and one slice (at a varying step) of every walk."""
    B = R.WALK << lp
    first, last = z0 // B, (z1 - 1) // B
    assert z0 % R.WALK and z0 % B and z1 % R.WALK and z1 % B, "the first and the last block are partial"
    assert len(set(interior)) >= 2 and all(first < b < last for b in interior)
    parts = [np.arange(z0, (first + 1) * B), np.arange(last * B, z1)]
    parts += [np.arange(b * B, (b + 1) * B) for b in interior]
    walks = np.arange(z0 // R.WALK, (z1 + R.WALK - 1) // R.WALK)
    parts.append(np.clip(walks * R.WALK + (walks * 37 + 11) % R.WALK, z0, z1 - 1))
    z = np.unique(np.concatenate(parts))
    assert np.array_equal(np.unique(z // R.WALK), walks) and z[0] == z0 and z[-1] == z1 - 1
    return z


# (form, set, slices, (per_wg, lp) the range must reach)
SHAPES = [
    ("i8", "dense5003", 8300, (2, 1)),
    ("i8", "dense5003", 66000, (16, 4)),   # 1.01 GiB
    ("c16", "dense5003", 2100, (2, 1)),
    ("c16", "dense5003", 16500, (16, 4)),  # 1.01 GiB
    ("i16", "c97_65", 8300, (2, 0)),       # 272 MB
    ("i32", "c33000", 8300, (2, 0)),       # 544 MB
]


@pytest.mark.parametrize("form,name,length,shape", SHAPES, ids=["%s-%d" % (c[0], c[2]) for c in SHAPES])
def test_production_launch_shapes(form, name, length, shape):
    torch = pytest.importorskip("torch")
    column_bits, elem_bytes = FORMS[form]
    z0, z1 = Z0, Z0 + length
    walks, per_wg, lp = R.launch_shape(column_bits, elem_bytes, z0, z1)
    assert (per_wg, lp) == shape
    B = R.WALK << lp
    first = z0 // B
    if elem_bytes == 1:  # one block per workgroup: the second block and a middle one
        interior = [first + 1, (first + (z1 - 1) // B) // 2]
    else:  # walks y, y + rows of one workgroup (y = 1): its first and its second, which reuses the stage
        rows = (walks + per_wg - 1) // per_wg
        assert per_wg == 2 and rows + 1 < walks - 1
        interior = [first + 1, first + 1 + rows]
    zs = sample(z0, z1, lp, interior)
    codes = dense5003_14() if form == "i8" else codes_of(form, name)
    with Plan(torch, form, codes) as p:
        buf = p.rows(z0, z1)
    assert bool((buf[z1 - z0] == FILL).all()), "bytes after the range were written"
    picked = torch.index_select(buf, 0, torch.from_numpy(zs - z0).cuda())
    del buf
    nbad, first_bad = 0, []
    for a in range(0, zs.size, 512):
        ref = R.rows_at(codes, column_bits, zs[a:a + 512])
        check_reference(ref, elem_bytes)
        n, f = differing(host_rows(picked[a:a + 512], elem_bytes), R.stored(ref, column_bits, elem_bytes),
                         zs[a:a + 512], elem_bytes)
        nbad, first_bad = nbad + n, (first_bad + f)[:8]
    print("%s %s [%d, %d): %d walks, %d per workgroup, blocks of %d; %d rows sampled, %d values differ"
          % (form, name, z0, z1, walks, per_wg, 1 << lp, zs.size, nbad))
    assert nbad == 0, first_bad


def _refused(torch, plan, row_bytes, z0, z1, out_bytes):
    buf = torch.full((2 * row_bytes,), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        plan.seed_rows(buf.data_ptr(), out_bytes, z0, z1)
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


@pytest.mark.parametrize("form", ["i16", "c16"])
def test_refuses_bad_ranges_and_sizes(form):
    torch = pytest.importorskip("torch")
    column_bits = FORMS[form][0]
    S = 1 << (32 - column_bits)
    with Plan(torch, form, codes_of(form, SETS[form][0])) as p:
        rb = p.row_bytes
        for z0, z1, nbytes in [(5, 5, 0), (6, 5, rb), (-1, 0, rb), (S - 1, S + 1, 2 * rb), (S, S + 1, rb),
                               (0, 1, rb - 1), (0, 1, 2 * rb), (0, 2, rb), (0, 1, rb // 2)]:
            _refused(torch, p.plan, rb, z0, z1, nbytes)
        if form == "c16":  # the 14-bit slice count is no bound here: 2^16 real slices
            _refused(torch, p.plan, rb, (1 << 18) - 1, 1 << 18, rb)


def test_refuses_other_plans():
    torch = pytest.importorskip("torch")
    codes = _sparse(500, 5)
    d_codes = torch.from_numpy(codes.view(np.int64)).cuda()
    for n, scheme in ((500, _lib.SCHEME_SUBSETS), (1, _lib.SCHEME_SPECTRAL)):
        plan = _lib.AllPairsPlan(d_codes.data_ptr(), n, 32, scheme=scheme)
        try:
            assert plan.scheme == scheme
            plan.build()
            _refused(torch, plan, 1 << 14, 0, 1, 1 << 14)
        finally:
            plan.close()
