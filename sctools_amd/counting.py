"""Counting observed barcodes on the GPU (no reference counterpart: the reference counts with
``collections.Counter`` on the host, barcode.py:100-102).

``DeviceCounter`` is a streaming ``Counter`` of encoded barcodes below 2**64: batches go in as
host arrays (``update``) or device pointers (``update_device``), and the distinct codes come
back with their counts in first-occurrence order -- the order ``Counter`` iterates in -- however
the device counted them (sctools_amd/csrc/count.hip).  Keys of 2**64 and above, and arbitrary
hashables, stay with the host ``Counter`` (``Barcodes.from_iterable_encoded``).
"""

import ctypes
from collections import Counter

import numpy as np

from . import _lib

__all__ = ["DeviceCounter"]

_vp, _i64 = ctypes.c_void_p, ctypes.c_int64


def _as_codes(codes):
    """(uint64 array, came-as-int64): np.uint64 as is, np.int64 viewed (a negative key is its
    two's-complement code and is viewed back on fetch), anything else through np.asarray."""
    if isinstance(codes, np.ndarray) and codes.dtype == np.int64:
        return np.ascontiguousarray(codes).reshape(-1).view(np.uint64), True
    if isinstance(codes, np.ndarray) and codes.dtype == np.uint64:
        return np.ascontiguousarray(codes).reshape(-1), False
    return np.ascontiguousarray(np.asarray(codes, dtype=np.uint64)).reshape(-1), False


class DeviceCounter:
    """A ``collections.Counter`` of uint64 codes kept on the device (sct_counter_*).

    ``capacity_hint`` sizes the first hash table; the table grows by itself.  Use as a context
    manager or ``close()`` it to free the device arrays."""

    def __init__(self, capacity_hint=1 << 20):
        self._lib = _lib.lib()
        self._h = _vp()
        self._signed = None  # dtype of the first host batch: int64 keys are viewed back on fetch
        _lib.check(self._lib.sct_counter_create(int(capacity_hint), ctypes.byref(self._h)))

    def update(self, codes):
        """Count a host batch (np.uint64 as is; np.int64 viewed as uint64; else converted)."""
        arr, signed = _as_codes(codes)
        if self._signed is None:
            self._signed = signed
        if arr.size:
            _lib.check(self._lib.sct_counter_update_host(self._h, _lib._ptr(arr), arr.size))
        return self

    def update_device(self, ptr, n, stream=0):
        """Count ``n`` uint64 codes at device pointer ``ptr`` (on ``stream``)."""
        if n:
            _lib.check(self._lib.sct_counter_update(self._h, _vp(ptr), int(n), _vp(stream)))
        return self

    def info(self):
        """dict(nunique, total, capacity)."""
        nu, tot, cap = _i64(0), _i64(0), _i64(0)
        _lib.check(self._lib.sct_counter_info(self._h, ctypes.byref(nu), ctypes.byref(tot), ctypes.byref(cap)))
        return {"nunique": nu.value, "total": tot.value, "capacity": cap.value}

    def __len__(self):
        return self.info()["nunique"]

    @property
    def total(self):
        """Codes seen so far."""
        tot = _i64(0)
        _lib.check(self._lib.sct_counter_info(self._h, None, ctypes.byref(tot), None))
        return tot.value

    def arrays(self, room=None):
        """(keys, counts uint64, first int64) of the distinct codes in first-occurrence order;
        keys are np.int64 when the counter was fed int64 arrays, else np.uint64.  ``room``
        (default: the number of distinct codes) sizes the output; too little raises ValueError."""
        got = len(self)
        n = got if room is None else int(room)
        keys = np.empty(n, np.uint64)
        counts = np.empty(n, np.uint64)
        first = np.empty(n, np.int64)
        _lib.check(self._lib.sct_counter_fetch_host(self._h, _lib._ptr(keys), _lib._ptr(counts), _lib._ptr(first), n))
        keys, counts, first = keys[:got], counts[:got], first[:got]
        return (keys.view(np.int64) if self._signed else keys), counts, first

    def fetch_device(self, keys_ptr, counts_ptr, first_ptr, room, stream=0):
        """The same rows into device arrays with room for ``room`` rows (sct_counter_fetch)."""
        _lib.check(self._lib.sct_counter_fetch(self._h, _vp(keys_ptr), _vp(counts_ptr), _vp(first_ptr), int(room),
                                               _vp(stream)))

    def counter(self):
        """``collections.Counter`` with Python-int keys and counts, iterating in the order
        ``Counter(all_codes.tolist())`` would."""
        keys, counts, _ = self.arrays()
        return Counter(dict(zip(keys.tolist(), counts.tolist())))

    def close(self):
        if self._h:
            self._lib.sct_counter_destroy(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
