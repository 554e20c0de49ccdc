"""The 16-bit-column tile (tile16_kernel in sctools_amd/csrc/spectral16.hip) labels every column
bit with a lane, register, tile or wave index and bins F^2 by the digit weight of that label;
test_gpu_tile_digits.py pins the 14-bit tile only, because small sets take 14-bit columns.  Here
the plan is forced to 16-bit columns (_lib.tuning(spectral_columns=16)): for every pair of column
bits i < j < 16 the set {0, 2^i | 2^j}, for every column bit i the sets {0, 2^i | 2^16} and
{0, 2^i | 2^31}, and small whitelists with duplicates and complements in three slice ranges --
each histogram must be the C oracle's."""
import numpy as np
import pytest

from oracle import oracle as O
from sctools_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

COLUMN_BITS = 16


def _spectral16_hist(torch, codes, ranges=None):
    d_codes = torch.from_numpy(codes.view(np.int64)).cuda()
    with _lib.tuning(spectral_columns=16):
        plan = _lib.AllPairsPlan(d_codes.data_ptr(), codes.size, 32, scheme=_lib.SCHEME_SPECTRAL)
    try:
        assert plan.scheme == _lib.SCHEME_SPECTRAL
        info = plan.spectral_info()
        assert info["column_bits"] == 16 and info["elem_bytes"] == 1, info
        counts = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
        credited = 0
        for b, e in ranges or [(0, plan.items)]:
            plan.build(0, b, e)
            plan.count(counts.data_ptr(), b, e)
            credited += plan.range_pairs(b, e)
        assert credited == codes.size * (codes.size - 1) // 2
        return plan.counts_to_hist(counts.cpu().numpy().view(np.uint64))
    finally:
        plan.close()


@pytest.mark.parametrize("i", range(COLUMN_BITS))
def test_two_code_sets_land_in_their_bin_16bit_columns(i):
    torch = pytest.importorskip("torch")
    for j in list(range(i + 1, COLUMN_BITS)) + [16, 31]:
        codes = np.array([0, (1 << i) | (1 << j)], dtype=np.uint64)
        ref = O.c_hist_rows(codes)[:17]
        want = np.zeros(17, np.int64)
        want[1 if i >> 1 == j >> 1 else 2] = 1
        assert ref.tolist() == want.tolist(), (i, j)
        hist = _spectral16_hist(torch, codes)
        print("bits (%d, %d): %s" % (i, j, hist.astype(np.int64).tolist()))
        assert hist.astype(np.int64).tolist() == ref.tolist(), (i, j)


@pytest.mark.parametrize("n", [2, 3, 5, 1025])
def test_forced_16bit_columns_match_oracle(n):
    """test_allpairs_spectral_scheme_matches_oracle's sets on 16-bit columns: nearly empty
    columns, duplicates (sum f^2 on this path) and complemented codes, in three slice ranges, one
    of them a single slice (virtual slices 1000..1001 are the 64-KiB slice 250)."""
    torch = pytest.importorskip("torch")
    codes = synthetic.whitelist_codes(max(2, n - n // 8), 16, seed=n + 7)
    extra = []
    if n >= 5:
        extra = [codes[0], codes[0], codes[1] ^ np.uint64(0xAAAAAAAA), codes[1] ^ np.uint64(0xFFFFFFFF)]
    codes = np.concatenate([codes, np.array(extra, dtype=np.uint64)])[:max(n, 2)]
    hist = _spectral16_hist(torch, codes, [(0, 1000), (1000, 1001), (1001, 1 << 18)])
    assert hist.astype(np.int64).tolist() == O.c_hist_rows(codes)[:17].tolist()
