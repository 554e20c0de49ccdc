"""CPU: the molecule counter's entry points (sct_molecules_*) reject bad arguments before they touch
a pointer or the device, fail loudly without a GPU, and the Python layer's names and argument checks
are in place.  No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import sctools_amd
from sctools_amd import _lib, counting

_ONE = (ctypes.c_uint64 * 4)()  # a valid host address where a non-NULL pointer is needed
_P = ctypes.cast(_ONE, ctypes.c_void_p)
_FAKE = ctypes.c_void_p(ctypes.addressof(_ONE))  # a non-NULL handle for checks that come before its use


def _invalid(rc, word):
    assert rc == _lib.SCT_E_INVALID
    assert word in _lib.last_error(), _lib.last_error()


def test_entries_reject_null_handle():
    lib = _lib.lib()
    _invalid(lib.sct_molecules_create(10, 3, 10, 64, None), "NULL")
    _invalid(lib.sct_molecules_update(None, _P, _P, 1, None), "counter is NULL")
    _invalid(lib.sct_molecules_update_host(None, _P, _P, 1), "counter is NULL")
    _invalid(lib.sct_molecules_info(None, None, None, None), "counter is NULL")
    _invalid(lib.sct_molecules_counts_host(None, _P, _P, _P), "counter is NULL")
    _invalid(lib.sct_molecules_counts(None, _P, _P, _P, None), "counter is NULL")
    _invalid(lib.sct_molecules_fetch_host(None, _P, _P, 1), "counter is NULL")
    _invalid(lib.sct_molecules_fetch(None, _P, _P, 1, None), "counter is NULL")
    assert lib.sct_molecules_destroy(None) == _lib.SCT_OK  # like free(NULL)


def test_entries_reject_negative_sizes_first():
    lib = _lib.lib()
    _invalid(lib.sct_molecules_update(None, _P, _P, -1, None), "n must be >= 0")
    _invalid(lib.sct_molecules_update_host(None, _P, _P, -1), "n must be >= 0")
    _invalid(lib.sct_molecules_fetch_host(None, _P, _P, -1), "room must be >= 0")
    _invalid(lib.sct_molecules_fetch(None, _P, _P, -1, None), "room must be >= 0")


def test_entries_reject_null_arrays():
    """The pointer checks come after the handle's and before the handle is used: a handle that is
    merely non-NULL gets as far as the message about the arrays."""
    lib = _lib.lib()
    _invalid(lib.sct_molecules_update(_FAKE, None, _P, 1, None), "NULL index or umi")
    _invalid(lib.sct_molecules_update(_FAKE, _P, None, 1, None), "NULL index or umi")
    _invalid(lib.sct_molecules_update_host(_FAKE, None, _P, 1), "NULL index or umi")
    _invalid(lib.sct_molecules_update_host(_FAKE, _P, None, 1), "NULL index or umi")
    _invalid(lib.sct_molecules_fetch_host(_FAKE, None, _P, 1), "NULL output")
    _invalid(lib.sct_molecules_fetch_host(_FAKE, _P, None, 1), "NULL output")
    # n == 0 changes nothing and needs no pointer
    assert lib.sct_molecules_update(_FAKE, None, None, 0, None) == _lib.SCT_OK
    assert lib.sct_molecules_update_host(_FAKE, None, None, 0) == _lib.SCT_OK


@pytest.mark.parametrize("nw, kind, L, word", [
    (0, 3, 10, "nw"),
    (2 ** 31, 2, 4, "nw"),
    (10, 4, 4, "kind"),
    (10, 3, 0, "L must be"),
    (2 ** 16, 2, 24, "63-bit key"),  # 16 index bits + 48 UMI bits = 64
])
def test_create_rejects(nw, kind, L, word):
    h = ctypes.c_void_p()
    _invalid(_lib.lib().sct_molecules_create(nw, kind, L, 64, ctypes.byref(h)), word)
    assert not h
    with pytest.raises(ValueError):
        counting.MoleculeCounter(nw, L, encoding=kind if kind in (2, 3) else "FourBit")


def test_create_rejects_capacity_hint():
    h = ctypes.c_void_p()
    _invalid(_lib.lib().sct_molecules_create(10, 3, 10, -1, ctypes.byref(h)), "capacity")
    _invalid(_lib.lib().sct_molecules_create(10, 3, 10, 2 ** 31 + 1, ctypes.byref(h)), "capacity")
    assert not h
    with pytest.raises(ValueError):
        counting.MoleculeCounter(10, 10, capacity_hint=-1)


def test_python_names_exist():
    assert sctools_amd.MoleculeCounter is counting.MoleculeCounter
    assert "MoleculeCounter" in counting.__all__
    for name in ("update", "update_device", "counts", "pairs", "info", "saturation", "close", "__len__", "__enter__",
                 "__exit__", "__del__"):
        assert hasattr(counting.MoleculeCounter, name), name
    for name in ("create", "update", "update_host", "info", "counts_host", "counts", "fetch_host", "fetch", "destroy"):
        assert "sct_molecules_" + name in _lib.SIGNATURES


def test_exact_conversion_of_host_arrays():
    a = np.array([0, -1, -2, 7], dtype=np.int32)
    assert counting._exact(a, np.int32, "index").dtype == np.int32
    assert counting._exact(np.array([0, -2, 2 ** 31 - 1], dtype=np.int64), np.int32, "index").tolist() == [0, -2, 2 ** 31 - 1]
    assert counting._exact([3, 2 ** 64 - 1], np.uint64, "umis").tolist() == [3, 2 ** 64 - 1]
    assert counting._exact([], np.uint64, "umis").size == 0
    for values, dtype in (([2 ** 31], np.int32), (np.array([-1], dtype=np.int64), np.uint64),
                          (np.array([1.5]), np.int32), (np.array([1.0]), np.uint64)):
        with pytest.raises(ValueError):
            counting._exact(values, dtype, "values")


def test_counter_without_gpu_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError):
        counting.MoleculeCounter(1000, 10)
