"""The SPECTRAL tile transform labels every column bit with a lane, register or tile index and
bins F^2 by the digit weight of that label.  A relabelling that pairs the wrong two bits into a
digit moves exactly the two-code sets below to another bin (or trips the host inversion's
checks): for every pair of column bits i < j < 14 the set {0, 2^i | 2^j}, and for every column
bit i the sets {0, 2^i | 2^14} and {0, 2^i | 2^31} (a column bit against the lowest and the
highest slice bit).  Each histogram must be the C oracle's: one pair, at distance 1 if both bits
share a 2-bit digit, else 2."""
import numpy as np
import pytest

from oracle import oracle as O
from sctools_amd import _lib

pytestmark = pytest.mark.gpu

COLUMN_BITS = 14


def _spectral_hist(torch, codes):
    d_codes = torch.from_numpy(codes.view(np.int64)).cuda()
    plan = _lib.AllPairsPlan(d_codes.data_ptr(), codes.size, 32, scheme=_lib.SCHEME_SPECTRAL)
    try:
        assert plan.scheme == _lib.SCHEME_SPECTRAL
        counts = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
        plan.build()
        plan.count(counts.data_ptr(), 0, plan.items)
        return plan.counts_to_hist(counts.cpu().numpy().view(np.uint64))
    finally:
        plan.close()


@pytest.mark.parametrize("i", range(COLUMN_BITS))
def test_two_code_sets_land_in_their_bin(i):
    torch = pytest.importorskip("torch")
    for j in list(range(i + 1, COLUMN_BITS)) + [14, 31]:
        codes = np.array([0, (1 << i) | (1 << j)], dtype=np.uint64)
        ref = O.c_hist_rows(codes)[:17]
        want = np.zeros(17, np.int64)
        want[1 if i >> 1 == j >> 1 else 2] = 1
        assert ref.tolist() == want.tolist(), (i, j)
        hist = _spectral_hist(torch, codes)
        print("bits (%d, %d): %s" % (i, j, hist.astype(np.int64).tolist()))
        assert hist.astype(np.int64).tolist() == ref.tolist(), (i, j)
