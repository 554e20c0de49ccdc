"""CPU: tests/seed_reference.py (the contract test_gpu_seed_rows.py holds the seed kernels to) against
independent restatements: rows against a direct +-1 sum over every (slice, column) of tiny code sets,
row_position against its rule bit by bit, launch_shape at the thresholds between launch geometries."""
import numpy as np
import pytest

import seed_reference as R

TINY = {
    "empty": [],
    "one": [0x2B5C],
    "pair_in_a_column": [(5 << 3) | 1, (6 << 3) | 1],
    "duplicates": [(3 << 3) | 7] * 5 + [(9 << 3) | 7, 0],
    "random": [int(v) for v in np.random.default_rng(3).integers(0, 1 << 9, 40)],
}


@pytest.mark.parametrize("name", sorted(TINY))
@pytest.mark.parametrize("column_bits", [3, 5])
def test_rows_against_direct_sum(name, column_bits):
    codes = TINY[name]
    nz = 1 << (14 - column_bits)  # past every code's high bits
    for z0, z1 in ((0, nz), (3, 11)):
        got = R.rows(np.array(codes, dtype=np.uint64), column_bits, z0, z1)
        assert got.dtype == np.int32 and got.shape == (z1 - z0, 1 << column_bits)
        for z in range(z0, z1):
            for c in range(1 << column_bits):
                want = sum((-1) ** bin((x >> column_bits) & z).count("1")
                           for x in codes if x & ((1 << column_bits) - 1) == c)
                assert got[z - z0, c] == want, (z, c)
    picked = [7, 0, 7, nz - 1]
    assert np.array_equal(R.rows_at(np.array(codes, dtype=np.uint64), column_bits, picked),
                          R.rows(np.array(codes, dtype=np.uint64), column_bits, 0, nz)[picked])


@pytest.mark.parametrize("elem_bytes", [1, 2, 4])
def test_row_position_is_its_rule_and_a_bijection(elem_bytes):
    L = {1: 4, 2: 3, 4: 2}[elem_bytes]
    # position bit i is column bit source[i]: the low L bits, bits 4..11, bits L..3, bits 12 and 13
    source = list(range(L)) + list(range(4, 12)) + list(range(L, 4)) + [12, 13]
    assert sorted(source) == list(range(14))
    c = np.arange(1 << 14)
    want = np.zeros_like(c)
    for i, b in enumerate(source):
        want |= ((c >> b) & 1) << i
    got = R.row_position(c, elem_bytes)
    assert np.array_equal(got, want)
    assert np.array_equal(np.sort(got), c)
    assert [R.row_position(int(v), elem_bytes) for v in (0, 8, 0x1AA0, 0x3FFF)] == [int(got[v]) for v in (0, 8, 0x1AA0, 0x3FFF)]
    if elem_bytes == 1:
        assert np.array_equal(got, c)
    else:
        assert got[8] != 8  # bit 3 moves


def test_stored_places_columns():
    ref = np.zeros((2, 1 << 14), np.int32)
    ref[0, 8], ref[1, 0x3FF7] = -300, 129
    for eb in (2, 4):
        s = R.stored(ref, 14, eb)
        assert s.dtype == R.DTYPES[eb]
        assert s[0, R.row_position(8, eb)] == -300 and s[1, R.row_position(0x3FF7, eb)] == 129
        assert np.count_nonzero(s) == 2
    with pytest.raises(AssertionError):
        R.stored(ref, 14, 1)  # 129 is no int8


def test_launch_shape_thresholds():
    S = 1 << 18
    assert R.launch_shape(14, 1, 1000, 3600) == (42, 1, 0)  # 2,600 slices from inside walk 15: walks 15..56
    assert R.launch_shape(14, 1, 0, 8192 - 64) == (127, 1, 0)
    assert R.launch_shape(14, 1, 0, 8192) == (128, 2, 1)
    assert R.launch_shape(14, 1, 0, 65536) == (1024, 16, 4)
    assert R.launch_shape(14, 1, 64 * 53 + 17, 64 * 53 + 17 + 65536) == (1025, 16, 4)
    assert R.launch_shape(14, 1, 0, 65535 - 64)[2] == 3
    assert R.launch_shape(14, 1, 0, S) == (4096, 16, 4)
    assert R.launch_shape(16, 1, 0, 2048 - 64) == (31, 1, 0)
    assert R.launch_shape(16, 1, 0, 2048) == (32, 2, 1)
    assert R.launch_shape(16, 1, 0, 16384) == (256, 16, 4)
    assert R.launch_shape(16, 1, 17, 17 + 16384) == (257, 16, 4)
    for eb in (2, 4):
        assert R.launch_shape(14, eb, 0, 8192 - 64) == (127, 1, 0)
        assert R.launch_shape(14, eb, 0, 8192) == (128, 2, 0)
        assert R.launch_shape(14, eb, 64 * 53 + 17, 64 * 53 + 17 + 8300) == (130, 2, 0)
        assert R.launch_shape(14, eb, 0, S) == (4096, 16, 0)
