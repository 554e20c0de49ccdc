"""CPU: sct_molecules_merge and sct_molecules_create_ex reject bad arguments before they touch a
counter or the device, and the Python layer's names are in place.  No kernel is launched here."""

import ctypes

import pytest

from sctools_amd import _lib, counting

_ONE = (ctypes.c_uint64 * 4)()
_FAKE = ctypes.c_void_p(ctypes.addressof(_ONE))  # a non-NULL handle for checks that come before its use


def _invalid(rc, word):
    assert rc == _lib.SCT_E_INVALID
    assert word in _lib.last_error(), _lib.last_error()


def test_merge_rejects_null_and_self():
    lib = _lib.lib()
    _invalid(lib.sct_molecules_merge(None, None, None), "counter is NULL")
    _invalid(lib.sct_molecules_merge(_FAKE, None, None), "counter is NULL")
    _invalid(lib.sct_molecules_merge(None, _FAKE, None), "counter is NULL")
    _invalid(lib.sct_molecules_merge(_FAKE, _FAKE, None), "itself")


@pytest.mark.parametrize("flags, device, word", [(2, -1, "flags"), (3, -1, "flags"), (-1, -1, "flags"),
                                                 (0, -2, "device"), (1, -7, "device")])
def test_create_ex_rejects_flags_and_device(flags, device, word):
    h = ctypes.c_void_p()
    _invalid(_lib.lib().sct_molecules_create_ex(10, 3, 10, 64, flags, device, ctypes.byref(h)), word)
    assert not h


def test_create_ex_keeps_creates_checks():
    """The parameter checks of sct_molecules_create come first, whatever flags and device say."""
    h = ctypes.c_void_p()
    lib = _lib.lib()
    _invalid(lib.sct_molecules_create_ex(10, 3, 10, 64, 0, -1, None), "NULL")
    _invalid(lib.sct_molecules_create_ex(0, 3, 10, 64, 1, 0, ctypes.byref(h)), "nw")
    _invalid(lib.sct_molecules_create_ex(10, 4, 4, 64, 1, 0, ctypes.byref(h)), "kind")
    _invalid(lib.sct_molecules_create_ex(2 ** 16, 2, 24, 64, 0, 0, ctypes.byref(h)), "63-bit key")
    _invalid(lib.sct_molecules_create_ex(10, 3, 10, -1, 0, 0, ctypes.byref(h)), "capacity")
    assert not h


def test_python_names_and_checks():
    for name in ("merge", "merge_device"):
        assert hasattr(counting.MoleculeCounter, name), name
    for name in ("merge", "create_ex"):
        assert "sct_molecules_" + name in _lib.SIGNATURES
    assert "merge_rows" in _lib.TUNE_KEYS
    with pytest.raises(ValueError, match="device"):
        counting.MoleculeCounter(10, 10, device=-1)
