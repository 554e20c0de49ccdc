"""CPU: the feature counter's entry points (include/sctools_hip.h, "counting molecules per feature")
reject bad arguments before they touch a pointer or the device, and the Python layer's names and
argument checks are in place.  No kernel is launched here."""

import ctypes

import pytest

from sctools_amd import _lib, counting

_ONE = (ctypes.c_uint64 * 4)()  # a valid host address where a non-NULL pointer is needed
_P = ctypes.cast(_ONE, ctypes.c_void_p)
_FAKE = ctypes.c_void_p(ctypes.addressof(_ONE))  # a non-NULL handle for checks that come before its use
_NNZ = ctypes.c_int64(-7)
_N = ctypes.byref(_NNZ)

NEW = ("create_features", "update_features", "update_features_host", "features_info", "fetch_features",
       "fetch_features_host", "matrix", "matrix_host")


def _invalid(rc, word):
    assert rc == _lib.SCT_E_INVALID
    assert word in _lib.last_error(), _lib.last_error()


def test_entries_reject_null_handle():
    lib = _lib.lib()
    _invalid(lib.sct_molecules_create_features(10, 4, 3, 10, 64, 0, -1, None), "NULL")
    _invalid(lib.sct_molecules_update_features(None, _P, _P, _P, 1, None), "counter is NULL")
    _invalid(lib.sct_molecules_update_features_host(None, _P, _P, _P, 1), "counter is NULL")
    _invalid(lib.sct_molecules_features_info(None, None, None), "counter is NULL")
    _invalid(lib.sct_molecules_fetch_features(None, _P, _P, _P, None, None, 1, None), "counter is NULL")
    _invalid(lib.sct_molecules_fetch_features_host(None, _P, _P, _P, None, None, 1), "counter is NULL")
    _invalid(lib.sct_molecules_matrix(None, _P, _P, _P, None, None, 1, _N, None), "counter is NULL")
    _invalid(lib.sct_molecules_matrix_host(None, _P, _P, _P, None, None, 1, _N), "counter is NULL")


def test_entries_reject_negative_sizes_first():
    lib = _lib.lib()
    _invalid(lib.sct_molecules_update_features(None, _P, _P, _P, -1, None), "n must be >= 0")
    _invalid(lib.sct_molecules_update_features_host(None, _P, _P, _P, -1), "n must be >= 0")
    _invalid(lib.sct_molecules_fetch_features(None, _P, _P, _P, None, None, -1, None), "room must be >= 0")
    _invalid(lib.sct_molecules_fetch_features_host(None, _P, _P, _P, None, None, -1), "room must be >= 0")
    _invalid(lib.sct_molecules_matrix(None, _P, _P, _P, None, None, -1, _N, None), "room must be >= 0")
    _invalid(lib.sct_molecules_matrix_host(None, _P, _P, _P, None, None, -1, _N), "room must be >= 0")


def test_entries_reject_null_arrays():
    """The pointer checks come after the handle's and before the handle is used: a handle that is
    merely non-NULL gets as far as the message about the arrays."""
    lib = _lib.lib()
    for hole in range(3):
        arrays = [None if k == hole else _P for k in range(3)]
        _invalid(lib.sct_molecules_update_features(_FAKE, *arrays, 1, None), "NULL index, feature or umi")
        _invalid(lib.sct_molecules_update_features_host(_FAKE, *arrays, 1), "NULL index, feature or umi")
        _invalid(lib.sct_molecules_fetch_features(_FAKE, *arrays, None, None, 1, None), "NULL output")
        _invalid(lib.sct_molecules_fetch_features_host(_FAKE, *arrays, None, None, 1), "NULL output")
    for indptr, feature in ((None, _P), (_P, None)):
        _invalid(lib.sct_molecules_matrix(_FAKE, indptr, feature, _P, None, None, 1, _N, None), "NULL output")
        _invalid(lib.sct_molecules_matrix_host(_FAKE, indptr, feature, _P, None, None, 1, _N), "NULL output")
    _invalid(lib.sct_molecules_matrix(_FAKE, _P, _P, _P, None, None, 1, None, None), "NULL nnz")
    _invalid(lib.sct_molecules_matrix_host(_FAKE, _P, _P, _P, None, None, 1, None), "NULL nnz")
    assert _NNZ.value == -7  # nothing was written on the way to an argument error
    # n == 0 changes nothing and needs no pointer
    assert lib.sct_molecules_update_features(_FAKE, None, None, None, 0, None) == _lib.SCT_OK
    assert lib.sct_molecules_update_features_host(_FAKE, None, None, None, 0) == _lib.SCT_OK


@pytest.mark.parametrize("nw, nf, kind, L, word", [
    (10, 0, 3, 10, "nf"),
    (10, -1, 3, 10, "nf"),
    (10, 2 ** 31, 2, 4, "nf"),
    (0, 4, 3, 10, "nw"),
    (10, 4, 4, 4, "kind"),
    (10, 4, 3, 0, "L must be"),
    (2 ** 16, 4, 2, 24, "63-bit key"),  # 16 index bits + 48 UMI bits: already too wide without features
    (737280, 8193, 3, 10, "index bits 20 + feature bits 14 + UMI bits 30"),  # the 64-bit key
    (2, 2, 2, 31, "index bits 1 + feature bits 1 + UMI bits 62"),
])
def test_create_rejects(nw, nf, kind, L, word):
    h = ctypes.c_void_p()
    _invalid(_lib.lib().sct_molecules_create_features(nw, nf, kind, L, 64, 0, -1, ctypes.byref(h)), word)
    assert not h
    with pytest.raises(ValueError):
        counting.MoleculeCounter(nw, L, encoding=kind if kind in (2, 3) else "FourBit", features=nf)


def test_create_rejects_flags_device_and_capacity():
    lib, h = _lib.lib(), ctypes.c_void_p()
    _invalid(lib.sct_molecules_create_features(10, 4, 3, 10, 64, 2, -1, ctypes.byref(h)), "flags")
    _invalid(lib.sct_molecules_create_features(10, 4, 3, 10, 64, 0, -2, ctypes.byref(h)), "device")
    _invalid(lib.sct_molecules_create_features(10, 4, 3, 10, -1, 0, -1, ctypes.byref(h)), "capacity")
    assert not h
    with pytest.raises(ValueError):
        counting.MoleculeCounter(10, 10, features=4, capacity_hint=-1)
    with pytest.raises(ValueError):
        counting.MoleculeCounter(10, 10, features=4, device=-3)


def test_python_names_exist():
    for name in ("matrix", "matrix_device", "features", "n_no_feature", "update", "update_device", "pairs"):
        assert hasattr(counting.MoleculeCounter, name), name
    for name in NEW:
        assert "sct_molecules_" + name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), "sct_molecules_" + name)
    import inspect
    assert "features" in inspect.signature(counting.MoleculeCounter.__init__).parameters
    assert "features" in inspect.signature(counting.MoleculeCounter.update).parameters
    assert "feature_ptr" in inspect.signature(counting.MoleculeCounter.update_device).parameters
    assert "features" in inspect.signature(counting.MoleculeCounter.pairs).parameters
    assert list(inspect.signature(counting.MoleculeCounter.matrix).parameters)[1:3] == ["reads", "collapsed"]
    # what existed keeps its order of arguments
    assert list(inspect.signature(counting.MoleculeCounter.__init__).parameters)[1:7] == [
        "whitelist_size", "umi_length", "encoding", "capacity_hint", "read_counts", "device"]
    assert list(inspect.signature(counting.MoleculeCounter.update_device).parameters)[1:5] == [
        "index_ptr", "umi_ptr", "n", "stream"]
    assert list(inspect.signature(counting.MoleculeCounter.pairs).parameters)[1:4] == ["room", "reads", "parents"]


def test_feature_counter_without_gpu_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError):
        counting.MoleculeCounter(1000, 10, features=16)
