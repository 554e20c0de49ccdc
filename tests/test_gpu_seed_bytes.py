"""The int8 SPECTRAL seed on 14-bit columns (seed_sm_kernel) against the formula, byte for byte:
seed(z, c) = sum over the codes of column c of (-1)^<code >> 14, z>.  A permutation of equal-weight
slices would leave every histogram unchanged, so the bytes are the check; sct_allpairs_seed_slices
writes them for any slice range into a caller's buffer.
  bytes   four code sets (columns of 0-3 codes; one column of 127 alone; neighbours of 64 and 65;
          5,003 random codes with 100 more in one column) x six slice ranges that start and end
          inside a 64-slice walk and cross walk and walk-block boundaries, the first and the last
          slice alone among them
  counts  plan.count over all 2^18 slices and over a three-way partition at non-aligned cuts: the
          same histogram, the C oracle's
  rule    plans with int16 seeds or 16-bit columns refuse the call
tools/seed_mx_ab.py runs the same byte check on the matrix-product seed of the timing variant."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from sctools_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

LO_BITS, LO = 14, 1 << 14
SLICES = 1 << 18
RANGES = [(0, 1), (0, 256), (255, 257), (777, 2277), (1000, 3600), (SLICES - 1, SLICES)]
CUTS = [0, 77777, 200001, SLICES]
FILL = 0x55  # the output buffers' content before the call (no whole row of seeds equals it: test_bytes)
SETS = ["sparse3000", "col127", "cols64_65", "dense5003"]


def _column(col, count, seed):
    """`count` distinct codes in 14-bit column `col`."""
    hi = np.random.default_rng(seed).choice(1 << 18, count, replace=False).astype(np.uint64)
    return (hi << np.uint64(LO_BITS)) | np.uint64(col)


@functools.lru_cache(maxsize=None)
def codes_of(name):
    if name == "sparse3000":  # columns of 0-3 codes
        return synthetic.whitelist_codes(3000, 16, seed=11)
    if name == "col127":  # one column of 127 codes alone: four groups, the int8 limit
        return _column(0x2B5C, 127, 21)
    if name == "cols64_65":  # neighbours: two groups exactly full, one code in the third
        return np.concatenate([_column(0x1234, 64, 22), _column(0x1235, 65, 23)])
    if name == "dense5003":  # 5,003 random codes and 100 more in one column
        return np.unique(np.concatenate([synthetic.whitelist_codes(5003, 16, seed=12), _column(0x3FF7, 100, 24)]))
    raise KeyError(name)


def _parity(x):
    x = x.copy()
    for s in (16, 8, 4, 2, 1):
        x ^= x >> np.uint32(s)
    return (x & np.uint32(1)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def formula(name, z0, z1):
    """[z1 - z0][2^14] int8: sum over the column's codes of (-1)^<h, z>."""
    codes = codes_of(name)
    col = (codes & np.uint64(LO - 1)).astype(np.int64)
    hi = (codes >> np.uint64(LO_BITS)).astype(np.uint32)
    z = np.arange(z0, z1, dtype=np.uint32)
    out = np.zeros((z1 - z0, LO), np.int32)
    for c in np.unique(col):
        h = hi[col == c]
        out[:, c] = (1 - 2 * _parity(h[None, :] & z[:, None])).sum(axis=1)
    assert np.abs(out).max() <= 127
    return out.astype(np.int8)


def _plan(torch, codes, **knobs):
    d_codes = torch.from_numpy(codes.view(np.int64)).cuda()
    with _lib.tuning(**knobs):
        plan = _lib.AllPairsPlan(d_codes.data_ptr(), codes.size, 32, scheme=_lib.SCHEME_SPECTRAL)
    assert plan.scheme == _lib.SCHEME_SPECTRAL
    return plan, d_codes


@functools.lru_cache(maxsize=None)
def seed_bytes(name):
    """The plan's seed bytes of every range of RANGES."""
    torch = pytest.importorskip("torch")
    plan, d_codes = _plan(torch, codes_of(name), spectral_chunk=4096)
    try:
        info = plan.spectral_info()
        assert (info["column_bits"], info["elem_bytes"]) == (LO_BITS, 1), info
        plan.build()
        out = []
        for z0, z1 in RANGES:
            buf = torch.full(((z1 - z0) * LO,), FILL, dtype=torch.int8, device="cuda")
            plan.seed_slices(buf.data_ptr(), z0, z1)
            torch.cuda.synchronize()
            out.append(buf.cpu().numpy().reshape(z1 - z0, LO))
        return out
    finally:
        plan.close()


@pytest.mark.parametrize("rng", range(len(RANGES)), ids=["%d-%d" % r for r in RANGES])
@pytest.mark.parametrize("name", SETS)
def test_bytes(name, rng):
    z0, z1 = RANGES[rng]
    want = formula(name, z0, z1)
    assert not (want == FILL).all(axis=1).any()  # an unwritten row cannot pass for a written one
    got = seed_bytes(name)[rng]
    bad = np.argwhere(got != want)
    print("%s [%d, %d): %d bytes, %d differ from the formula" % (name, z0, z1, want.size, len(bad)))
    assert len(bad) == 0, [(int(z) + z0, int(c), int(got[z, c]), int(want[z, c])) for z, c in bad[:8]]


@pytest.mark.parametrize("name", ["sparse3000", "dense5003"])
def test_counts_whole_and_in_three_parts(name):
    torch = pytest.importorskip("torch")
    assert all(c % 64 for c in CUTS[1:-1])
    ref = [int(v) for v in O.c_hist_rows(codes_of(name))[:17]]
    plan, d_codes = _plan(torch, codes_of(name))
    try:
        plan.build()
        whole = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
        plan.count(whole.data_ptr(), 0, plan.items)
        parts = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            plan.count(parts.data_ptr(), a, b)
        for c in (whole, parts):
            assert [int(v) for v in plan.counts_to_hist(c.cpu().numpy().view(np.uint64))] == ref
    finally:
        plan.close()


@pytest.mark.parametrize("columns", [14, 16])
def test_other_seeds_refuse(columns):
    """int16 seeds (one 14-bit column of 200 codes) and 16-bit columns: no int8 rows of 2^14 to write."""
    torch = pytest.importorskip("torch")
    codes = np.concatenate([_column(0x0AAA, 200, 31), synthetic.whitelist_codes(500, 16, seed=5)])
    plan, d_codes = _plan(torch, codes, spectral_columns=columns)
    try:
        info = plan.spectral_info()
        assert (info["column_bits"], info["elem_bytes"]) == ((14, 2) if columns == 14 else (16, 1)), info
        plan.build()
        buf = torch.full((LO,), FILL, dtype=torch.int8, device="cuda")
        with pytest.raises(ValueError):
            plan.seed_slices(buf.data_ptr(), 0, 1)
        torch.cuda.synchronize()
        assert bool((buf == FILL).all())
    finally:
        plan.close()
