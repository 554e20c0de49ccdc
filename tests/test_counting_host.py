"""CPU: the counting entry points (sct_counter_*, sct_index_tally, sct_nearest_*count_host) reject
bad arguments before they touch a pointer or the device, fail loudly without a GPU, and the Python
layer's names and its int64 <-> uint64 key view are in place.  No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import sctools_amd
from sctools_amd import _lib, barcode, counting

_ONE = (ctypes.c_uint64 * 4)()  # a valid host address where a non-NULL pointer is needed
_P = ctypes.cast(_ONE, ctypes.c_void_p)
_H = ctypes.c_void_p()


def _invalid(rc, word):
    assert rc == _lib.SCT_E_INVALID
    assert word in _lib.last_error(), _lib.last_error()


def test_counter_entries_reject_null_handle():
    lib = _lib.lib()
    _invalid(lib.sct_counter_create(64, None), "NULL")
    _invalid(lib.sct_counter_update(None, _P, 1, None), "NULL")
    _invalid(lib.sct_counter_update_host(None, _P, 1), "NULL")
    _invalid(lib.sct_counter_info(None, None, None, None), "NULL")
    _invalid(lib.sct_counter_fetch_host(None, _P, _P, _P, 1), "NULL")
    _invalid(lib.sct_counter_fetch(None, _P, _P, _P, 1, None), "NULL")
    assert lib.sct_counter_destroy(None) == _lib.SCT_OK  # like free(NULL)


def test_counter_entries_reject_negative_sizes():
    lib = _lib.lib()
    h = ctypes.c_void_p()
    _invalid(lib.sct_counter_create(-1, ctypes.byref(h)), "capacity")
    assert not h
    _invalid(lib.sct_counter_update(None, _P, -1, None), "n must be >= 0")
    _invalid(lib.sct_counter_update_host(None, _P, -1), "n must be >= 0")
    _invalid(lib.sct_counter_fetch_host(None, _P, _P, _P, -1), "room must be >= 0")
    _invalid(lib.sct_counter_fetch(None, _P, _P, _P, -1, None), "room must be >= 0")


def test_index_tally_rejects_bad_arguments():
    lib = _lib.lib()
    _invalid(lib.sct_index_tally(_P, -1, 4, _P, _P, None), ">= 0")
    _invalid(lib.sct_index_tally(_P, 1, -1, _P, _P, None), ">= 0")
    _invalid(lib.sct_index_tally(_P, 1, 4, None, _P, None), "NULL")
    _invalid(lib.sct_index_tally(_P, 1, 4, _P, None, None), "NULL")
    _invalid(lib.sct_index_tally(None, 1, 4, _P, _P, None), "NULL")
    assert lib.sct_index_tally(None, 0, 4, _P, _P, None) == _lib.SCT_OK  # nothing to count


def test_nearest_count_rejects_bad_arguments():
    lib = _lib.lib()
    for f in (lib.sct_nearest_count_host, lib.sct_nearest_multi_count_host):
        _invalid(f(None, _P, 1, _P, _P), "NULL")
        _invalid(f(None, _P, -1, _P, _P), "nq must be >= 0")


def test_counter_without_gpu_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError):
        counting.DeviceCounter()
    with pytest.raises(RuntimeError):
        barcode.Barcodes.from_encoded_array(np.arange(10, dtype=np.uint64), 16)


def test_python_names_exist():
    assert sctools_amd.DeviceCounter is counting.DeviceCounter
    assert sctools_amd.counting is counting
    for name in ("update", "update_device", "arrays", "counter", "close", "total", "__len__", "__enter__"):
        assert hasattr(counting.DeviceCounter, name), name
    for cls in (barcode.Barcodes, barcode.ObservedBarcodeSet, barcode.PriorBarcodeSet):
        assert callable(cls.from_encoded_array)
    assert callable(barcode.WhitelistCorrector.count)
    assert callable(_lib.HostNearestPlan.count)
    assert _lib.TUNE_KEYS["count_preagg"] == 17


def test_empty_whitelist_count_needs_no_device():
    wc = barcode.WhitelistCorrector(np.zeros(0, dtype=np.uint64))
    counts, n_none, n_tie = wc.count(np.arange(5, dtype=np.uint64))
    assert counts.shape == (0,) and counts.dtype == np.int64
    assert (n_none, n_tie) == (5, 0)
    counts, n_none, n_tie = wc.count(np.arange(3, dtype=np.uint64), out=(counts, n_none, n_tie))
    assert (n_none, n_tie) == (8, 0)
    with pytest.raises(ValueError):
        wc.count(np.arange(3, dtype=np.uint64), out=np.zeros(2, dtype=np.int64))


def test_int64_keys_round_trip_through_the_uint64_view():
    """Negative int64 keys go to the device as their two's-complement uint64 codes and come back
    through the inverse view: the same values, and distinct keys stay distinct."""
    keys = np.array([-1, -2, 0, 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, -12345], dtype=np.int64)
    as_codes, signed = counting._as_codes(keys)
    assert signed and as_codes.dtype == np.uint64
    assert as_codes.tolist() == [k % 2 ** 64 for k in keys.tolist()]
    assert np.array_equal(as_codes.view(np.int64), keys)
    assert len(set(as_codes.tolist())) == keys.size
    u = np.array([0, 2 ** 64 - 1, 2 ** 63], dtype=np.uint64)
    same, signed = counting._as_codes(u)
    assert not signed and same.dtype == np.uint64 and same.tolist() == u.tolist()
    lst, signed = counting._as_codes([3, 2 ** 64 - 1])
    assert not signed and lst.dtype == np.uint64 and lst.tolist() == [3, 2 ** 64 - 1]
