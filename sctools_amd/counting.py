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

__all__ = ["DeviceCounter", "MoleculeCounter", "ReadGroups", "remove_swapped"]

# the status of a read under ReadGroups.tag (include/sctools_hip.h, SCT_READ_*)
GROUPED, NO_BARCODE, AMBIGUOUS, BAD_UMI, NO_FEATURE, ABSENT, LOST, BAD_INDEX = range(8)

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


def _exact(values, dtype, what):
    """``values`` as a flat contiguous array of ``dtype``: as is when it has that dtype, else
    converted only if every value survives the round trip (ValueError otherwise)."""
    if isinstance(values, np.ndarray) and values.dtype == dtype:
        return np.ascontiguousarray(values).reshape(-1)
    # (a Python sequence is looked at as objects: numpy would make [3, 2**64 - 1] a float array)
    src = values if isinstance(values, np.ndarray) else np.asarray(values, dtype=object)
    if src.size:
        lim = np.iinfo(dtype)
        whole = src.dtype.kind in "iub" or (src.dtype.kind == "O" and all(
            isinstance(v, (int, np.integer)) for v in src.reshape(-1).tolist()))
        if not whole or int(src.min()) < lim.min or int(src.max()) > lim.max:
            raise ValueError("%s: %s values do not all fit %s" % (what, src.dtype.name, np.dtype(dtype).name))
    return np.ascontiguousarray(src.astype(dtype)).reshape(-1)


COLLAPSE_METHODS = {"one_step": _lib.COLLAPSE_ONE_STEP, "directional": _lib.COLLAPSE_DIRECTIONAL}


def collapse_method(name):
    """The SCT_COLLAPSE_* number of a collapse method's name: 'one_step' (every UMI to its best
    neighbour, once) or 'directional' (UMI-tools' directional clusters).  Anything else raises
    ValueError."""
    if not isinstance(name, str) or name not in COLLAPSE_METHODS:
        raise ValueError("method must be 'one_step' or 'directional', not %r" % (name,))
    return COLLAPSE_METHODS[name]


RESOLVE_METHODS = dict(COLLAPSE_METHODS, none=_lib.COLLAPSE_NONE)


def resolve_method(name):
    """The SCT_COLLAPSE_* number of a method's name for ``resolve`` and ``matrix(resolved=True)``:
    ``collapse_method``'s two, or 'none' (every UMI is its own molecule).  Anything else raises
    ValueError."""
    if not isinstance(name, str) or name not in RESOLVE_METHODS:
        raise ValueError("method must be 'one_step', 'directional' or 'none', not %r" % (name,))
    return RESOLVE_METHODS[name]


def downsample_threshold(fraction):
    """The integer threshold in [0, 2**32] of a fraction of the reads in [0, 1]:
    ``int(round(fraction * 2**32))``.  The scaling by a power of two is exact, so a fraction always
    maps to the same threshold.  Anything outside [0, 1] (nan included) raises ValueError."""
    f = float(fraction)
    if not 0.0 <= f <= 1.0:
        raise ValueError("fraction must lie in [0, 1], not %r" % (fraction,))
    return int(round(f * 4294967296))


def _seed(value, what="seed"):
    """``value`` as a ctypes uint64; ValueError unless it is an int in [0, 2**64)."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) < 2 ** 64:
        raise ValueError("%s must be an int in [0, 2**64), not %r" % (what, value))
    return ctypes.c_uint64(int(value))


def _fraction(min_fraction):
    """``min_fraction`` as (num, den): a pair of ints with 1 <= num <= den <= 2**32 and 2 * num > den
    (include/sctools_hip.h, "removing swapped molecules"); ValueError otherwise.  Not a float: the
    judgement is exact."""
    try:
        num, den = min_fraction
    except (TypeError, ValueError):
        raise ValueError("min_fraction must be a pair of ints (num, den), not %r" % (min_fraction,)) from None
    for v in (num, den):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("min_fraction must be a pair of ints (num, den), not %r" % (min_fraction,))
    num, den = int(num), int(den)
    if not (1 <= num <= den <= 2 ** 32 and 2 * num > den):
        raise ValueError("min_fraction %d / %d must have 1 <= num <= den <= 2**32 and 2 * num > den" % (num, den))
    return num, den


def _check_swapped(samples, targets):
    """What sct_molecules_swapped asks of the samples of a lane and of the counters their kept
    molecules go into, in merge_device's pattern: TypeError for a non-counter; ValueError for a wrong
    number of samples, a closed or repeated counter, a target among the samples, missing
    ``read_counts`` or parameters that differ from the first sample's."""
    for c in samples + targets:
        if not isinstance(c, MoleculeCounter):
            raise TypeError("remove_swapped needs MoleculeCounters, not %s" % type(c).__name__)
    if not 1 <= len(samples) <= 16:
        raise ValueError("remove_swapped takes 1 to 16 samples, not %d" % len(samples))
    for c in samples + targets:
        if not c._h:
            raise ValueError("remove_swapped: %s counter is closed" % ("a target" if c in targets else "a sample's"))
    if len({id(c) for c in samples + targets}) != len(samples) + len(targets):
        raise ValueError("remove_swapped: a counter is repeated among the samples and targets")
    for c in samples + targets:
        c._need_read_counts("remove_swapped")
    first = samples[0]
    mine = (first.size, first.kind, first.umi_length, first._nf)
    for c in samples[1:] + targets:
        theirs = (c.size, c.kind, c.umi_length, c._nf)
        for name, a, b in zip(("whitelist_size", "encoding", "umi_length", "features"), mine, theirs):
            if a != b:
                raise ValueError("remove_swapped: the counters' %s differ (%r and %r)" % (name, a, b))


def remove_swapped(counters, min_fraction=(4, 5), into=None):
    """The samples of one lane without the molecules that hopped between them (DropletUtils'
    ``swappedDrops``, on the device): ``counters`` is a sequence of 1 to 16 ``MoleculeCounter`` with
    ``read_counts``, equal whitelist_size, umi_length, encoding and features, on one device.  A
    (barcode, UMI[, feature]) seen in several of them stays in the sample that holds at least
    ``min_fraction`` = (num, den) of its reads and leaves every other one; when no sample reaches the
    fraction all lose it.  No UMI collapse is applied first; ``collapse`` works on the results.

    Returns (cleaned, tally): ``cleaned[k]`` is a new counter like ``counters[k]`` holding its kept
    molecules, with its reads, tallies and total -- an ordinary counter -- or, with ``into=`` (a list
    of as many counters), ``into[k]`` after the kept molecules were added to it.  ``tally`` is
    np.int64[(len(counters), 3)]: per sample the shared molecules, the removed ones and the removed
    reads.  The sources are not changed.  TypeError for anything but counters; ValueError for a closed
    or repeated counter, differing parameters, missing ``read_counts`` or a bad fraction; counters
    made by the call are closed when it fails."""
    num, den = _fraction(min_fraction)
    counters = list(counters)
    made = into is None
    into = [] if made else list(into)
    if not made and len(into) != len(counters):
        raise ValueError("remove_swapped: into= holds %d counters for %d samples" % (len(into), len(counters)))
    _check_swapped(counters, into)  # every check before any sample is judged: a failure changes nothing
    tally = np.zeros((len(counters), 3), np.int64)
    try:
        for k, c in enumerate(counters):
            if made:
                # (the smallest table: the call grows it to what survives)
                into.append(MoleculeCounter(c.size, c.umi_length, encoding={3: 'ThreeBit', 2: 'TwoBit'}[c.kind],
                                            capacity_hint=0, read_counts=True, device=c.device, features=c._nf))
            tally[k] = c.remove_swapped_device(counters[:k] + counters[k + 1:], into[k], num, den)
    except Exception:
        if made:
            for c in into:
                c.close()
        raise
    return into, tally


class MoleculeCounter:
    """Molecules per whitelist barcode on the device (sct_molecules_*): the distinct
    (corrected barcode index, UMI code) pairs, which removes PCR duplicates.

    ``whitelist_size`` barcodes (1 .. 2**31 - 1), UMIs of ``umi_length`` bases in ``encoding``
    ('ThreeBit' or 'TwoBit'); the index bits and the UMI bits must fit a 63-bit key.  Feed it the
    ``index`` of ``WhitelistCorrector.correct`` / ``nearest`` and the encoded UMIs of the same
    reads.  ``capacity_hint`` sizes the first table; it grows by itself.  Use as a context manager
    or ``close()`` it to free the device arrays.

    ``read_counts=True`` also keeps the reads of every molecule (8 more bytes per table slot), which
    ``collapse()``, ``pairs(reads=True)`` and ``saturation(collapsed=True)`` need: they merge a UMI
    into the best-supported UMI one base away under the same barcode (include/sctools_hip.h,
    "collapsing UMIs one base apart").

    ``device`` is the HIP ordinal the counter lives on (default: the device current when it is
    made).  Every method works whatever device is current and leaves it as it was; device pointers
    and streams given to the ``*_device`` methods belong to the counter's device.  Counters fed
    different pieces of the reads -- one per file or lane, or one per GPU -- become one with
    ``merge``.  With ``read_counts``, ``downsample(fraction)`` gives the counter a fraction of the
    reads would have made, and ``saturation_curve(fractions)`` the reads and molecules at every depth
    in one pass (include/sctools_hip.h, "downsampling reads").  The counters of the samples of one
    lane are cleaned of the molecules that hopped between them by ``remove_swapped`` (this module's
    function; include/sctools_hip.h, "removing swapped molecules").

    ``features=nf`` (1 .. 2**31 - 1) makes a *feature counter*: every read carries a feature index
    (an antibody tag or guide corrected by ``WhitelistCorrector``, or a gene index) as a third key
    part, the same UMI under two features of a cell is two molecules, and ``matrix()`` returns the
    barcode x feature molecules as CSR (include/sctools_hip.h, "counting molecules per feature").
    Index, feature and UMI bits must fit a 63-bit key together.  With ``read_counts`` as well,
    ``resolve()`` and ``matrix(resolved=True)`` give a (barcode, UMI) seen under several features to
    the one with the most reads and drop it on a tie (include/sctools_hip.h, "resolving features")."""

    def __init__(self, whitelist_size, umi_length, encoding='ThreeBit', capacity_hint=1 << 20, read_counts=False,
                 device=None, features=None):
        kinds = {'ThreeBit': 3, 'TwoBit': 2, 3: 3, 2: 2}
        if encoding not in kinds:
            raise ValueError("encoding must be 'ThreeBit' or 'TwoBit'")
        nw, L, kind = int(whitelist_size), int(umi_length), kinds[encoding]
        if not 1 <= nw < 2 ** 31:
            raise ValueError("whitelist_size %d outside [1, 2**31)" % nw)
        if L < 1:
            raise ValueError("umi_length must be >= 1")
        idx_bits = max(1, (nw - 1).bit_length())
        if idx_bits + kind * L > 63:
            raise ValueError("index bits %d + UMI bits %d do not fit a 63-bit key" % (idx_bits, kind * L))
        nf = None if features is None else int(features)
        if nf is not None:
            if not 1 <= nf < 2 ** 31:
                raise ValueError("features %d outside [1, 2**31)" % nf)
            feat_bits = max(1, (nf - 1).bit_length())
            if idx_bits + feat_bits + kind * L > 63:
                raise ValueError("index bits %d + feature bits %d + UMI bits %d do not fit a 63-bit key"
                                 % (idx_bits, feat_bits, kind * L))
        if not 0 <= int(capacity_hint) <= 2 ** 31:
            raise ValueError("capacity_hint outside [0, 2**31]")
        self.size, self.umi_length, self.kind = nw, L, kind
        self._nf = nf
        self._lib = _lib.lib()
        self._h = _vp()
        self.read_counts = bool(read_counts)
        self.device = None if device is None else int(device)
        if self.device is not None and self.device < 0:
            raise ValueError("device must be a HIP ordinal (or None for the current device)")
        dev = -1 if self.device is None else self.device
        if nf is None:
            _lib.check(self._lib.sct_molecules_create_ex(nw, kind, L, int(capacity_hint), int(self.read_counts), dev,
                                                         ctypes.byref(self._h)))
        else:
            _lib.check(self._lib.sct_molecules_create_features(nw, nf, kind, L, int(capacity_hint),
                                                               int(self.read_counts), dev, ctypes.byref(self._h)))

    @property
    def features(self):
        """The number of features of a feature counter, else None."""
        return self._nf

    @property
    def n_no_feature(self):
        """Reads that had a barcode and a good UMI but a feature of -1 or -2 (0 without features)."""
        n = _i64(0)
        _lib.check(self._lib.sct_molecules_features_info(self._h, None, ctypes.byref(n)))
        return n.value

    def _need_features(self, what):
        if self._nf is None:
            raise ValueError("%s needs MoleculeCounter(..., features=nf)" % what)

    def _need_read_counts(self, what):
        if not self.read_counts:
            raise ValueError("%s needs MoleculeCounter(..., read_counts=True)" % what)

    def update(self, index, umis, features=None):
        """Count a host batch: ``index`` int32 (-1 no match, -2 ambiguous, else a whitelist index)
        and the reads' uint64 UMI codes.  An index outside [-2, whitelist_size) raises ValueError
        after the rest of the batch was counted.  A feature counter needs ``features`` as well, int32
        of the same length (-1 / -2: no feature; outside [-2, nf) raises like a bad index); any
        other counter rejects it."""
        if (features is None) != (self._nf is None):
            raise ValueError("update: features= is %s" % ("needed by a feature counter" if features is None
                                                          else "only taken by MoleculeCounter(..., features=nf)"))
        idx = _exact(index, np.int32, "index")
        umi = _exact(umis, np.uint64, "umis")
        if idx.size != umi.size:
            raise ValueError("index and umis differ in length: %d vs %d" % (idx.size, umi.size))
        if features is None:
            if idx.size:
                _lib.check(self._lib.sct_molecules_update_host(self._h, _lib._ptr(idx), _lib._ptr(umi), idx.size))
            return self
        feat = _exact(features, np.int32, "features")
        if feat.size != idx.size:
            raise ValueError("index and features differ in length: %d vs %d" % (idx.size, feat.size))
        if idx.size:
            _lib.check(self._lib.sct_molecules_update_features_host(self._h, _lib._ptr(idx), _lib._ptr(feat),
                                                                    _lib._ptr(umi), idx.size))
        return self

    def update_device(self, index_ptr, umi_ptr, n, stream=0, feature_ptr=None):
        """Count ``n`` reads from device pointers (int32 indices, uint64 UMI codes and, for a feature
        counter, int32 features at ``feature_ptr``) on ``stream``."""
        if (feature_ptr is None) != (self._nf is None):
            raise ValueError("update_device: feature_ptr= is %s" % (
                "needed by a feature counter" if feature_ptr is None
                else "only taken by MoleculeCounter(..., features=nf)"))
        if not n:
            return self
        if feature_ptr is None:
            _lib.check(self._lib.sct_molecules_update(self._h, _vp(index_ptr), _vp(umi_ptr), int(n), _vp(stream)))
        else:
            _lib.check(self._lib.sct_molecules_update_features(self._h, _vp(index_ptr), _vp(feature_ptr), _vp(umi_ptr),
                                                               int(n), _vp(stream)))
        return self

    def counts(self):
        """(reads, molecules, n_none, n_ambiguous, n_bad_umi): np.int64[whitelist_size] twice --
        reads and distinct molecules per barcode -- and the reads that had no barcode, an ambiguous
        one, or a barcode and a bad UMI."""
        reads = np.empty(self.size, np.uint64)
        molecules = np.empty(self.size, np.uint64)
        tally = np.empty(3, np.uint64)
        _lib.check(self._lib.sct_molecules_counts_host(self._h, _lib._ptr(reads), _lib._ptr(molecules), _lib._ptr(tally)))
        return (reads.view(np.int64), molecules.view(np.int64), int(tally[0]), int(tally[1]), int(tally[2]))

    def pairs(self, room=None, reads=False, parents=False, features=False, method='one_step'):
        """(index int32, umi uint64) of the distinct molecules, ascending by index, then by UMI code.
        ``room`` (default: the number of molecules) sizes the output; too little raises ValueError.
        ``reads=True`` (a counter with ``read_counts``) adds each molecule's reads (int64), and
        ``parents=True`` with it the UMI each molecule collapses into (its own if it stays).
        ``features=True`` (a feature counter): (index, feature int32, umi[, reads][, parents]),
        ascending by index, then feature, then UMI code.  ``method='directional'``: the parents column
        carries each molecule's root (``collapse``)."""
        by = collapse_method(method)
        if parents and not reads:
            raise ValueError("parents=True needs reads=True")
        if reads:
            self._need_read_counts("pairs(reads=True)")
        if features:
            self._need_features("pairs(features=True)")
        got = len(self)
        n = got if room is None else int(room)
        index, umi = np.empty(n, np.int32), np.empty(n, np.uint64)
        feature = np.empty(n, np.int32) if features else None
        mreads = np.empty(n, np.uint64) if reads else None
        parent = np.empty(n, np.uint64) if parents else None
        p = _lib._ptr
        if features:
            _lib.check(self._lib.sct_molecules_fetch_features_by_host(self._h, by, p(index), p(feature), p(umi),
                                                                      p(mreads), p(parent), n))
        elif reads:
            _lib.check(self._lib.sct_molecules_fetch_counted_by_host(self._h, by, p(index), p(umi), p(mreads),
                                                                     p(parent), n))
        else:
            _lib.check(self._lib.sct_molecules_fetch_host(self._h, p(index), p(umi), n))
        columns = (index, feature, umi, mreads.view(np.int64) if reads else None, parent)
        return tuple(col[:got] for col in columns if col is not None)

    def fetch_device(self, index_ptr, umi_ptr, room, stream=0):
        """The same rows into device arrays with room for ``room`` rows (sct_molecules_fetch)."""
        _lib.check(self._lib.sct_molecules_fetch(self._h, _vp(index_ptr), _vp(umi_ptr), int(room), _vp(stream)))

    def fetch_counted_device(self, index_ptr, umi_ptr, reads_ptr, parent_ptr, room, stream=0, method='one_step'):
        """fetch_device's rows with uint64 reads and, unless ``parent_ptr`` is 0 / None, uint64 parent
        UMIs beside them (sct_molecules_fetch_counted_by); ``method='directional'`` writes the roots
        there and may wait for ``stream``."""
        by = collapse_method(method)
        self._need_read_counts("fetch_counted_device")
        _lib.check(self._lib.sct_molecules_fetch_counted_by(self._h, by, _vp(index_ptr), _vp(umi_ptr), _vp(reads_ptr),
                                                            _vp(parent_ptr or None), int(room), _vp(stream)))

    def matrix(self, reads=False, collapsed=False, room=None, method='one_step', resolved=False):
        """The barcode x feature count matrix of a feature counter as CSR: (indptr int64
        [whitelist_size + 1], feature int32 [nnz], molecules int64 [nnz]) and, if asked (a counter
        with ``read_counts``), reads and collapsed (int64 [nnz]) after them -- the entry's reads and
        its molecules after the UMI collapse.  Features ascend within a row, and
        ``scipy.sparse.csr_matrix((molecules, feature, indptr), shape=(whitelist_size, features))``
        takes the arrays as they are.  ``room`` (default: the number of molecules, which always
        suffices) sizes the output; fewer than nnz raises ValueError, which names nnz.
        ``method='directional'``: collapsed is the entry's directional clusters (``collapse``).
        ``resolved=True`` (a counter with ``read_counts``) adds a last column, the entry's molecules
        that ``resolve(method)`` keeps; ``method`` may then be 'none' as well, but not together with
        ``collapsed``.  The column shares indptr and feature with the others, so an entry that loses
        every molecule holds an explicit 0 (``scipy``'s ``eliminate_zeros()`` drops those)."""
        by = resolve_method(method) if resolved else collapse_method(method)
        self._need_features("matrix")
        if reads:
            self._need_read_counts("matrix(reads=True)")
        if collapsed:
            self._need_read_counts("matrix(collapsed=True)")
        if resolved:
            self._need_read_counts("matrix(resolved=True)")
            if collapsed and by == _lib.COLLAPSE_NONE:
                raise ValueError("matrix(collapsed=True) needs a collapse method, not 'none'")
        n = len(self) if room is None else int(room)
        if n < 0:
            raise ValueError("room must be >= 0")
        indptr = np.empty(self.size + 1, np.int64)
        feature = np.empty(max(n, 1), np.int32)
        values = [np.empty(max(n, 1), np.uint64) if want else None for want in (True, reads, collapsed, resolved)]
        nnz = _i64(0)
        if resolved:
            _lib.check(self._lib.sct_molecules_matrix_resolved_host(
                self._h, by, _lib._ptr(indptr), _lib._ptr(feature), _lib._ptr(values[0]), _lib._ptr(values[1]),
                _lib._ptr(values[2]), _lib._ptr(values[3]), None, n, ctypes.byref(nnz)))
        else:
            _lib.check(self._lib.sct_molecules_matrix_by_host(self._h, by, _lib._ptr(indptr), _lib._ptr(feature),
                                                              _lib._ptr(values[0]), _lib._ptr(values[1]),
                                                              _lib._ptr(values[2]), n, ctypes.byref(nnz)))
        k = nnz.value
        return (indptr, feature[:k].copy()) + tuple(v[:k].view(np.int64).copy() for v in values if v is not None)

    def matrix_device(self, indptr_ptr, feature_ptr, molecules_ptr, reads_ptr, collapsed_ptr, room, stream=0,
                      method='one_step', resolved_ptr=None):
        """matrix() into device arrays with room for ``room`` entries (sct_molecules_matrix_by): int64
        [whitelist_size + 1], int32 [room] and up to three uint64 [room], each of the three 0 / None
        when not wanted.  Returns nnz; waits for ``stream`` once to learn it.  ``resolved_ptr`` (not
        0 / None): one more uint64 [room], matrix(resolved=True)'s last column
        (sct_molecules_matrix_resolved); ``method`` may then be 'none'."""
        by = resolve_method(method) if resolved_ptr else collapse_method(method)
        self._need_features("matrix_device")
        if reads_ptr or collapsed_ptr:
            self._need_read_counts("matrix_device with reads or collapsed")
        nnz = _i64(0)
        if resolved_ptr:
            self._need_read_counts("matrix_device with resolved")
            if collapsed_ptr and by == _lib.COLLAPSE_NONE:
                raise ValueError("matrix_device with collapsed needs a collapse method, not 'none'")
            _lib.check(self._lib.sct_molecules_matrix_resolved(
                self._h, by, _vp(indptr_ptr), _vp(feature_ptr or None), _vp(molecules_ptr or None),
                _vp(reads_ptr or None), _vp(collapsed_ptr or None), _vp(resolved_ptr), None, int(room),
                ctypes.byref(nnz), _vp(stream)))
            return nnz.value
        _lib.check(self._lib.sct_molecules_matrix_by(self._h, by, _vp(indptr_ptr), _vp(feature_ptr or None),
                                                     _vp(molecules_ptr or None), _vp(reads_ptr or None),
                                                     _vp(collapsed_ptr or None), int(room), ctypes.byref(nnz),
                                                     _vp(stream)))
        return nnz.value

    def collapse(self, method='one_step'):
        """(collapsed np.int64[whitelist_size], n_corrected int): the molecules per barcode after every
        UMI went to the best-supported UMI one base away (ties to the larger code), and how many moved.
        ``method='directional'`` is UMI-tools' directional method instead: a UMI with a reads joins a
        UMI one base away with b reads when b >= 2 * a - 1, transitively; collapsed counts the
        clusters per barcode and n_corrected the molecules that are not their cluster's root
        (include/sctools_hip.h, "directional clusters")."""
        by = collapse_method(method)
        self._need_read_counts("collapse")
        collapsed = np.empty(self.size, np.uint64)
        ncorr = np.zeros(1, np.uint64)
        _lib.check(self._lib.sct_molecules_collapse_by_host(self._h, by, _lib._ptr(collapsed), _lib._ptr(ncorr)))
        return collapsed.view(np.int64), int(ncorr[0])

    def resolve(self, method='one_step'):
        """(resolved np.int64[whitelist_size], n_shared, n_lost, n_tied, reads_dropped) of a feature
        counter with ``read_counts``: a (barcode, UMI) seen under several features is one molecule, so
        after the UMI collapse of ``method`` ('one_step', 'directional', or 'none' for no collapse)
        the feature with the most reads keeps it and the others lose it; on a tie for the most reads
        every feature of the group drops it.  resolved counts the kept molecules per barcode,
        n_shared the (barcode, UMI) groups under two or more features, n_lost and n_tied the
        molecules discarded either way and reads_dropped their reads (include/sctools_hip.h,
        "resolving features").  ``matrix(resolved=True)`` gives the kept molecules per entry."""
        by = resolve_method(method)
        self._need_features("resolve")
        self._need_read_counts("resolve")
        resolved = np.empty(self.size, np.uint64)
        tally = np.zeros(4, np.uint64)
        _lib.check(self._lib.sct_molecules_resolve_host(self._h, by, _lib._ptr(resolved), _lib._ptr(tally)))
        return (resolved.view(np.int64),) + tuple(int(t) for t in tally)

    def resolve_device(self, resolved_ptr, tally_ptr=None, stream=0, method='one_step'):
        """resolve() into device memory: uint64[whitelist_size] and, unless 0 / None, uint64[4]
        (sct_molecules_resolve), on ``stream``; ``method='directional'`` may wait for it."""
        by = resolve_method(method)
        self._need_features("resolve_device")
        self._need_read_counts("resolve_device")
        _lib.check(self._lib.sct_molecules_resolve(self._h, by, _vp(resolved_ptr), _vp(tally_ptr or None),
                                                   _vp(stream)))

    def collapse_device(self, collapsed_ptr, ncorrected_ptr=None, stream=0, method='one_step'):
        """collapse() into device memory: uint64[whitelist_size] and, unless 0 / None, one uint64
        (sct_molecules_collapse_by), on ``stream``; ``method='directional'`` may wait for it."""
        by = collapse_method(method)
        self._need_read_counts("collapse_device")
        _lib.check(self._lib.sct_molecules_collapse_by(self._h, by, _vp(collapsed_ptr), _vp(ncorrected_ptr or None),
                                                       _vp(stream)))

    def merge_device(self, other, stream=0):
        """``merge`` enqueued on ``stream`` (of this counter's device; sct_molecules_merge): it waits
        for the earlier work of both counters on any stream, and their later work waits for it."""
        if not isinstance(other, MoleculeCounter):
            raise TypeError("merge needs a MoleculeCounter, not %s" % type(other).__name__)
        if other is self:
            raise ValueError("a MoleculeCounter cannot be merged into itself")
        if not self._h or not other._h:
            raise ValueError("merge: %s counter is closed" % ("this" if not self._h else "the other"))
        mine = (self.size, self.kind, self.umi_length, self.read_counts, self._nf)
        theirs = (other.size, other.kind, other.umi_length, other.read_counts, other._nf)
        for name, a, b in zip(("whitelist_size", "encoding", "umi_length", "read_counts", "features"), mine, theirs):
            if a != b:
                raise ValueError("merge: the counters' %s differ (%r and %r)" % (name, a, b))
        _lib.check(self._lib.sct_molecules_merge(self._h, other._h, _vp(stream)))
        return self

    def merge(self, other):
        """Add another counter to this one, on the device: afterwards this counter is what it would
        be had it been fed its own reads and then ``other``'s -- reads, molecules (the union: a
        molecule seen by both counts once), tallies, total, per-molecule reads, and so ``collapse()``.
        ``other`` must have the same whitelist_size, umi_length, encoding and read_counts; it may live
        on another device, is not changed and stays usable.  The table grows first if it has to.
        TypeError for anything but a MoleculeCounter; ValueError for this counter itself, a closed
        counter or differing parameters.  Returns self."""
        return self.merge_device(other)

    def downsample_device(self, into, threshold, seed=0, stream=0):
        """``downsample`` enqueued on ``stream`` with the threshold as an integer in [0, 2**32]
        (sct_molecules_downsample): read j of a molecule is kept when its draw lies below it.  Waits
        for ``stream`` to learn how many molecules survive.  Returns ``into``."""
        self._need_read_counts("downsample")
        if not isinstance(into, MoleculeCounter):
            raise TypeError("downsample needs a MoleculeCounter to thin into, not %s" % type(into).__name__)
        if into is self:
            raise ValueError("a MoleculeCounter cannot be downsampled into itself")
        if not self._h or not into._h:
            raise ValueError("downsample: %s counter is closed" % ("this" if not self._h else "the target"))
        into._need_read_counts("downsample(into=...)")
        mine = (self.size, self.kind, self.umi_length, self._nf)
        theirs = (into.size, into.kind, into.umi_length, into._nf)
        for name, a, b in zip(("whitelist_size", "encoding", "umi_length", "features"), mine, theirs):
            if a != b:
                raise ValueError("downsample: the counters' %s differ (%r and %r)" % (name, a, b))
        _lib.check(self._lib.sct_molecules_downsample(into._h, self._h, _seed(threshold, "threshold"), _seed(seed),
                                                      _vp(stream)))
        return into

    def downsample(self, fraction, seed=0, into=None):
        """This counter with every read kept with probability ``fraction``, added to ``into`` (default:
        a new counter of the same whitelist_size, umi_length, encoding, features and device, with
        ``read_counts``) and returned: binomial thinning of each molecule's reads, the molecules that
        keep none dropped, the tallies thinned alike (include/sctools_hip.h, "downsampling reads").
        The result is an ordinary counter -- ``collapse``, ``matrix``, ``merge`` work on it -- sized for
        what survives.  What is kept depends on ``seed`` (an int in [0, 2**64)), the molecule and the
        read's number only: equal counters thin to equal tables whatever their history, and a smaller
        fraction keeps a subset of a larger one's reads.  This counter is not changed."""
        self._need_read_counts("downsample")
        threshold = downsample_threshold(fraction)
        made = into is None
        if made:
            into = MoleculeCounter(self.size, self.umi_length, encoding={3: 'ThreeBit', 2: 'TwoBit'}[self.kind],
                                   read_counts=True, device=self.device, features=self._nf)
        try:
            return self.downsample_device(into, threshold, seed)
        except Exception:
            if made:
                into.close()
            raise

    def remove_swapped_device(self, others, into, num, den, stream=0):
        """This sample's molecules that the ``others`` (the lane's other samples, a sequence of at
        most 15 counters) do not take from it, added to ``into`` on ``stream``
        (sct_molecules_swapped): a molecule with r reads here and t in the others together is kept
        when r / (r + t) >= num / den.  Returns np.int64[3]: this sample's shared molecules, the
        removed ones and the reads of the removed ones.  Waits for ``stream`` once."""
        num, den = _fraction((num, den))
        samples = [self] + list(others)
        _check_swapped(samples, [into])
        handles = (_vp * len(samples))(*[c._h for c in samples])
        tally = np.zeros(3, np.uint64)
        _lib.check(self._lib.sct_molecules_swapped(handles, len(samples), 0, into._h, num, den, _lib._ptr(tally),
                                                   _vp(stream)))
        return tally.view(np.int64)

    def saturation_curve_device(self, thresholds, reads_ptr, molecules_ptr, seed=0, stream=0):
        """``saturation_curve`` into device memory, on ``stream``: ``thresholds`` is a non-decreasing
        sequence of 1 to 64 integers in [0, 2**32], and uint64[len(thresholds)] is written at each
        pointer that is not 0 / None (sct_molecules_downsample_curve)."""
        self._need_read_counts("saturation_curve")
        th = np.array([_seed(t, "threshold").value for t in thresholds], dtype=np.uint64)
        _lib.check(self._lib.sct_molecules_downsample_curve(self._h, _lib._ptr(th), th.size, _seed(seed),
                                                            _vp(reads_ptr or None), _vp(molecules_ptr or None),
                                                            _vp(stream)))

    def saturation_curve(self, fractions, seed=0):
        """(reads, molecules), each np.int64[len(fractions)]: the reads kept and the molecules still
        seen at every one of 1 to 64 non-decreasing ``fractions`` of the reads, in one pass over the
        table -- ``counts()[0].sum()`` and ``counts()[1].sum()`` of ``downsample(f, seed)`` for each f.
        Sequencing saturation at depth f is ``1 - molecules / reads``."""
        self._need_read_counts("saturation_curve")
        th = np.array([downsample_threshold(f) for f in fractions], dtype=np.uint64)
        reads, molecules = np.empty(th.size, np.uint64), np.empty(th.size, np.uint64)
        _lib.check(self._lib.sct_molecules_downsample_curve_host(self._h, _lib._ptr(th), th.size, _seed(seed),
                                                                 _lib._ptr(reads), _lib._ptr(molecules)))
        return reads.view(np.int64), molecules.view(np.int64)

    def read_groups(self, method='one_step', resolved=False, reads=False, first=False):
        """A ``ReadGroups`` snapshot of this counter under ``method`` ('none', 'one_step' or
        'directional'): ``tag`` then gives every read its corrected UMI and status on the device."""
        return ReadGroups(self, method=method, resolved=resolved, reads=reads, first=first)

    def info(self):
        """dict(nmolecules, total, capacity)."""
        nm, tot, cap = _i64(0), _i64(0), _i64(0)
        _lib.check(self._lib.sct_molecules_info(self._h, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cap)))
        return {"nmolecules": nm.value, "total": tot.value, "capacity": cap.value}

    def __len__(self):
        return self.info()["nmolecules"]

    def saturation(self, collapsed=False, method='one_step'):
        """Sequencing saturation 1 - molecules / reads over the counted reads (nan when none);
        ``collapsed=True`` takes the molecules of ``collapse(method)``."""
        collapse_method(method)
        reads, molecules = self.counts()[:2]
        if collapsed:
            molecules = self.collapse(method=method)[0]
        total = int(reads.sum())
        return 1.0 - int(molecules.sum()) / total if total else float("nan")

    def close(self):
        if self._h:
            self._lib.sct_molecules_destroy(self._h)
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


class ReadGroups:
    """Every read tagged with its molecule (sct_read_groups_*; include/sctools_hip.h, "read groups"):
    a snapshot of a ``MoleculeCounter``'s molecules under a collapse ``method`` ('none', 'one_step' or
    'directional', the names ``resolve`` takes), against which batches of reads -- the same pieces
    ``update`` was fed, in any order -- are tagged on the device.

    ``resolved=True`` (a feature counter with ``read_counts``): reads of the molecules that
    ``resolve(method)`` discards get the status LOST.  ``reads=True`` (``read_counts``) adds the reads
    of every read's final molecule, ``first=True`` marks the first read of every molecule over all
    the reads tagged so far (duplicate marking).  'one_step' and 'directional' need ``read_counts``.

    The object describes the counter as it stood when it was made and owns what it reads: the counter
    may be updated, merged into or closed afterwards.  It lives on the counter's device; every method
    works whatever device is current.  Use as a context manager or ``close()`` it."""

    def __init__(self, counter, method='one_step', resolved=False, reads=False, first=False):
        if not isinstance(counter, MoleculeCounter):
            raise TypeError("ReadGroups needs a MoleculeCounter, not %s" % type(counter).__name__)
        self._h = _vp()
        by = resolve_method(method)
        if not counter._h:
            raise ValueError("read_groups: the counter is closed")
        if by != _lib.COLLAPSE_NONE:
            counter._need_read_counts("read_groups(method=%r)" % method)
        if resolved:
            counter._need_features("read_groups(resolved=True)")
            counter._need_read_counts("read_groups(resolved=True)")
        if reads:
            counter._need_read_counts("read_groups(reads=True)")
        self.method, self.resolved, self.reads, self.first = method, bool(resolved), bool(reads), bool(first)
        self._nf = counter._nf
        self.device = counter.device
        self._lib = counter._lib
        flags = (_lib.GROUPS_RESOLVED * self.resolved | _lib.GROUPS_READS * self.reads
                 | _lib.GROUPS_FIRST * self.first)
        _lib.check(self._lib.sct_read_groups_create(counter._h, by, flags, ctypes.byref(self._h), None))

    def _handle(self):
        if not self._h:
            raise ValueError("the read groups are closed")
        return self._h

    def tag(self, index, umis, features=None):
        """Tag a host batch: ``index`` int32, the reads' uint64 UMI codes and, for a feature
        counter's groups, int32 ``features`` (rejected otherwise), as ``update`` takes them.  Returns
        (final_umi uint64, status uint8[, mol_reads int64 with ``reads``][, first bool with
        ``first``]) per read; the statuses are this module's GROUPED .. BAD_INDEX.  A BAD_INDEX read
        raises ValueError after the whole batch was tagged."""
        if (features is None) != (self._nf is None):
            raise ValueError("tag: features= is %s" % ("needed by a feature counter's read groups" if features is None
                                                       else "only taken by MoleculeCounter(..., features=nf)"))
        idx = _exact(index, np.int32, "index")
        umi = _exact(umis, np.uint64, "umis")
        if idx.size != umi.size:
            raise ValueError("index and umis differ in length: %d vs %d" % (idx.size, umi.size))
        feat = None
        if features is not None:
            feat = _exact(features, np.int32, "features")
            if feat.size != idx.size:
                raise ValueError("index and features differ in length: %d vs %d" % (idx.size, feat.size))
        n = idx.size
        final, status = np.empty(n, np.uint64), np.empty(n, np.uint8)
        mreads = np.empty(n, np.uint64) if self.reads else None
        first = np.empty(n, np.uint8) if self.first else None
        h, p = self._handle(), _lib._ptr
        if n:
            _lib.check(self._lib.sct_read_groups_tag_host(h, p(idx), p(feat), p(umi), n, p(final), p(status),
                                                          p(mreads), p(first)))
        columns = (final, status, mreads.view(np.int64) if self.reads else None,
                   first.view(np.bool_) if self.first else None)
        return tuple(col for col in columns if col is not None)

    def tag_device(self, index_ptr, umi_ptr, n, final_umi_ptr, status_ptr, reads_ptr=None, first_ptr=None,
                   feature_ptr=None, stream=0):
        """Tag ``n`` reads from device pointers into device pointers, on ``stream`` (sct_read_groups_tag):
        uint64 final UMIs, uint8 statuses and, exactly when the groups were made with them, uint64
        reads and uint8 first flags.  Waits for ``stream`` once; a BAD_INDEX read raises ValueError
        after the whole batch was tagged."""
        if (feature_ptr is None) != (self._nf is None):
            raise ValueError("tag_device: feature_ptr= is %s" % (
                "needed by a feature counter's read groups" if feature_ptr is None
                else "only taken by MoleculeCounter(..., features=nf)"))
        h = self._handle()
        if n:
            _lib.check(self._lib.sct_read_groups_tag(h, _vp(index_ptr), _vp(feature_ptr), _vp(umi_ptr), int(n),
                                                     _vp(final_umi_ptr), _vp(status_ptr), _vp(reads_ptr or None),
                                                     _vp(first_ptr or None), _vp(stream)))
        return self

    def tally(self):
        """np.int64[8]: the reads per status over everything tagged so far."""
        out = np.zeros(8, np.uint64)
        _lib.check(self._lib.sct_read_groups_info(self._handle(), None, _lib._ptr(out)))
        return out.view(np.int64)

    @property
    def tagged(self):
        """Reads given to ``tag`` / ``tag_device`` so far."""
        n = _i64(0)
        _lib.check(self._lib.sct_read_groups_info(self._handle(), ctypes.byref(n), None))
        return n.value

    def close(self):
        if self._h:
            self._lib.sct_read_groups_destroy(self._h)
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
