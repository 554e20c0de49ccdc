"""The reference of the saturating code families (spectral_families.py) is the C oracle on the
distinct codes, scaled: hist = m^2 * hist(distinct) (+ #distinct * m (m - 1) / 2 at 0).  Checked
here against the oracle on the expanded multiset at a size where that is quick, with the
properties of the families the GPU tests rely on."""
import numpy as np
import pytest

import spectral_families as F
from oracle import oracle as O


@pytest.mark.parametrize("kind", ["mask0", "ones", "bit3", "neg", "rand"])
def test_family_hist_is_the_oracle_on_the_expanded_multiset(kind):
    bits, m = 10, 5  # 10-bit "columns": 5120 codes
    e = 1 | (1 << (31 - bits))
    if kind == "rand":
        distinct = F.random_sign_distinct(bits, seed=4)
    else:
        mask = {"mask0": 0, "ones": (1 << bits) - 1, "bit3": 8, "neg": 8}[kind]
        distinct = F.saturating_distinct(bits, mask, e, neg=kind == "neg")
    assert np.array_equal(distinct & np.uint64((1 << bits) - 1), np.arange(1 << bits, dtype=np.uint64))
    assert np.unique(distinct).size == 1 << bits and int(distinct.max()) < 1 << 32
    codes = F.expand(distinct, m, shuffle_seed=1)
    n = codes.size
    assert n == m << bits
    ref = F.family_hist(distinct, m)
    assert ref == O.c_hist_rows(codes)[:17].tolist()
    assert sum(ref) == n * (n - 1) // 2


@pytest.mark.parametrize("bits", [14, 16])
def test_family_shapes(bits):
    """Every column holds exactly m codes; the slice parts are 0 / e by the mask's parity."""
    e = 1 | (1 << (31 - bits))
    mask = (1 << 6) | 1
    for neg in (False, True):
        d = F.saturating_distinct(bits, mask, e, neg)
        c = np.arange(1 << bits)
        par = np.array([bin(v & mask).count("1") & 1 for v in c]) ^ int(neg)
        assert np.array_equal(d >> np.uint64(bits), (par * e).astype(np.uint64))
    codes = F.expand(F.saturating_distinct(bits, mask, e), 127)
    assert np.array_equal(np.bincount((codes & np.uint64((1 << bits) - 1)).astype(np.int64)), np.full(1 << bits, 127))
    h = F.random_sign_distinct(bits, seed=1) >> np.uint64(bits)
    assert set(np.unique(h).tolist()) == set(F.slice_span(bits).tolist()) and len(set(F.slice_span(bits).tolist())) == 8
    assert int(F.slice_span(bits).max()) < 1 << (32 - bits)
