"""Counting on the device against the host ways of getting the same answer, on one box in one run.

Input A (the corrected-flow shape): config 4's observed ThreeBit codes (synthetic.config4_queries
against the 737,280 whitelist).  Input B (the worst case for a hash table): 3,686,400 pairwise
distinct codes followed by the same array again -- every key new, then every key a hit.
Per input and per pre-aggregation mode (SCT_TUNE_COUNT_PREAGG 0 none / 1 wave merge / 2 LDS table;
interleaved rounds in one process): DeviceCounter.update_device time, the table's growth, nunique
and the fraction of 8 TB/s the 8 B/code read reaches; the host-resident update; and the yardsticks
Counter(codes.tolist()) and np.unique(codes, return_index=True, return_counts=True), whose reduced
n is stated.  Then WhitelistCorrector.count against .nearest() + np.bincount on one batch, with
the bytes each moves over PCIe.  Then MoleculeCounter.update_device on 100M (index, UMI) reads
against DeviceCounter on composite keys plus sct_index_tally, with a molecule's reads far apart and
adjacent (molecules_step; its rounds also go to profiles/ab_molecules_<tag>.jsonl).  Then, on the same
reads, the counted MoleculeCounter and its UMI collapse against the plain one, an earlier library and
the host (collapse_step; profiles/ab_umi_collapse_<tag>.jsonl).  Then MoleculeCounter.merge of the
second half's counter into the first's against an update of as many reads as the source has molecules
and against the host route, with the existing molecule rows again beside an earlier library
(merge_step; profiles/ab_molecules_merge_<tag>.jsonl).  Then the same reads with a feature column
(nf = 4096): update_features against the plain update, matrix_device in its three forms, the host
route pairs(features=True) + np.unique, and the plain and counted updates beside an earlier library
(matrix_step; profiles/ab_count_matrix.jsonl, or ab_count_matrix_<tag>.jsonl for a tag other than
"run").  Then the calls that read a table back, merge two and grow one, each beside an earlier library,
timings and outputs (calls_step; profiles/ab_molecules_calls_<tag>.jsonl).  Then the directional
clusters in both forms beside the one-step collapse, on the same reads with --umi-error substitutions
per UMI base, and the updates and the one-step collapse beside an earlier library (directional_step;
profiles/ab_umi_directional.jsonl).  Then downsampling on the same reads: downsample at two fractions,
the saturation curve, merge and the host route beside them, SCT_TUNE_DOWNSAMPLE_WAVE_READS swept on a
skewed table, and the updates, the collapse and the merge beside an earlier library (downsample_step;
profiles/ab_downsample.jsonl).  Then resolving features on the matrix step's reads with --hop of them
moved to another feature: resolve_device for the three methods, the resolved matrix, the matrix as it
was and the host route pairs() + np.lexsort + reduceat, device and host answers equal, and the matrix
call beside an earlier library (resolve_step; profiles/ab_feature_resolve.jsonl).  Then read groups on
the same input: read_groups() for every method, tag_device with each set of columns beside
update_features of the same reads, the host route pairs() + np.searchsorted + np.lexsort + np.unique
with equal answers, and the updates, collapse, resolve and matrix beside an earlier library
(groups_step; profiles/ab_read_groups.jsonl).  Then removing swapped molecules: the molecules step's
reads split over 2 and 4 counters with --hop of them moved to another sample, remove_swapped per
sample and whole beside the merge of the same counters, the host route pairs() + np.unique +
np.searchsorted with equal answers, and the existing calls beside an earlier library (swapped_step;
profiles/ab_swapped.jsonl).

Every step runs in a child process of its own under its own time limit; a step that fails ends
the run.  One short JSON line on stdout; the detail goes to profiles/count_<tag>.json.

  python tools/bench_count.py --tag mi355x
  python tools/bench_count.py --tag mi355x --only molecules
  python tools/bench_count.py --tag mi355x --only collapse --parent-lib /path/to/earlier/libsctools_hip.so
  python tools/bench_count.py --tag mi355x --only merge --parent-lib /path/to/earlier/libsctools_hip.so
  python tools/bench_count.py --only matrix --parent-lib /path/to/earlier/libsctools_hip.so
  python tools/bench_count.py --only calls --parent-lib /path/to/earlier/libsctools_hip.so
  python tools/bench_count.py --only directional --umi-error 0.01 --parent-lib /path/to/earlier/libsctools_hip.so
  python tools/bench_count.py --only downsample --parent-lib /path/to/earlier/libsctools_hip.so
  python tools/bench_count.py --only resolve --hop 0.02 --parent-lib /path/to/earlier/libsctools_hip.so
  python tools/bench_count.py --only groups --hop 0.02 --parent-lib /path/to/earlier/libsctools_hip.so
  python tools/bench_count.py --only swapped --hop 0.02 --parent-lib /path/to/earlier/libsctools_hip.so
"""
import argparse
import functools
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"counter_A": 420, "counter_B": 300, "tally": 300, "molecules": 420, "collapse": 600,
         "merge": 600, "matrix": 600, "calls": 600, "directional": 600, "downsample": 600,
         "resolve": 900, "groups": 1100, "swapped": 1100}  # seconds
MODES = {0: "none", 1: "wave_merge", 2: "lds_table"}
HBM_BYTES_PER_S = 8e12


def _time_ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def counter_step(which, args):
    import numpy as np
    import torch
    from sctools_amd import _lib, counting, synthetic

    if which == "A":
        n, L, seed = synthetic.CONFIGS[4]
        wl3 = synthetic.two_to_three(synthetic.whitelist_codes(n, L, seed), L)
        d, _, _ = synthetic.config4_queries(wl3, args.n_a, seed=4, device=torch.device("cuda"))
    else:
        n, L, seed = synthetic.CONFIGS[5]
        once = synthetic.whitelist_codes(n, L, seed)
        d = torch.from_numpy(np.concatenate([once, once]).view(np.int64)).cuda()
    torch.cuda.synchronize()
    n = d.numel()
    out = {"input": which, "n": n, "modes": {}}

    def run_device(mode):
        with _lib.tuning(count_preagg=mode):
            dc = counting.DeviceCounter()
            cap0 = dc.info()["capacity"]

            def go():
                dc.update_device(d.data_ptr(), n)
                torch.cuda.synchronize()
            ms = _time_ms(go)
            info = dc.info()
            dc.close()
        return ms, cap0, info

    run_device(1)  # warm-up: code objects, pool
    times = {m: [] for m in MODES}
    for _ in range(args.rounds):
        for m in MODES:
            ms, cap0, info = run_device(m)
            times[m].append(ms)
            out["nunique"] = info["nunique"]
            out["capacity_start"], out["capacity_end"] = cap0, info["capacity"]
    out["growth_doublings"] = (out["capacity_end"] // out["capacity_start"]).bit_length() - 1
    for m, name in MODES.items():
        med = float(np.median(times[m]))
        out["modes"][name] = {"update_device_ms": [round(t, 3) for t in times[m]], "median_ms": round(med, 3),
                              "min_ms": round(min(times[m]), 3),
                              "read_fraction_of_8TBps": round(n * 8 / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
    # a table sized up front (no growth on the way): what the growth costs
    with counting.DeviceCounter(capacity_hint=out["capacity_end"]) as dc:
        def go():
            dc.update_device(d.data_ptr(), n)
            torch.cuda.synchronize()
        out["presized_update_device_ms"] = round(_time_ms(go), 3)
        out["fetch_host_ms"] = round(_time_ms(dc.arrays), 3)
    codes = d.cpu().numpy().view(np.uint64)
    with counting.DeviceCounter() as dc:
        out["update_host_ms"] = round(_time_ms(lambda: dc.update(codes)), 3)
        assert len(dc) == out["nunique"] and dc.total == n
        if which == "B":
            keys, counts, first = dc.arrays()
            assert keys.size == n // 2 and (counts == 2).all() and np.array_equal(first, np.arange(n // 2))
    # the host ways to the same answer (reduced n, stated; the Python loop is linear in n)
    nc = min(n, args.n_counter)
    from collections import Counter
    sub = codes[:nc]
    t = _time_ms(lambda: Counter(sub.tolist()))
    out["host_counter"] = {"n": nc, "ms": round(t, 1), "ns_per_code": round(t * 1e6 / nc, 1)}
    nu = min(n, args.n_unique)
    sub = codes[:nu]
    t = _time_ms(lambda: np.unique(sub, return_index=True, return_counts=True))
    out["host_np_unique"] = {"n": nu, "ms": round(t, 1), "ns_per_code": round(t * 1e6 / nu, 1)}
    best = min(v["median_ms"] for v in out["modes"].values())
    out["device_ns_per_code_best"] = round(best * 1e6 / n, 4)
    return out


def tally_step(args):
    import numpy as np
    import torch
    from sctools_amd import _lib, barcode, synthetic

    n, L, seed = synthetic.CONFIGS[4]
    wl3 = synthetic.two_to_three(synthetic.whitelist_codes(n, L, seed), L)
    d, _, _ = synthetic.config4_queries(wl3, args.n_tally, seed=4, device=torch.device("cuda"))
    q = _lib.pinned.empty(args.n_tally, np.uint64)  # page-locked, as the encoder returns its codes
    q[:] = d.cpu().numpy().view(np.uint64)
    del d
    wc = barcode.WhitelistCorrector(wl3, max_distance=1, encoding="ThreeBit")

    def old():
        idx, _ = wc.nearest(q)
        idx = np.asarray(idx)
        return np.bincount(idx[idx >= 0], minlength=wc.size), int((idx == -1).sum()), int((idx == -2).sum())

    ref = old()
    got = wc.count(q)
    assert np.array_equal(got[0], ref[0]) and got[1:] == ref[1:]
    t_old, t_near, t_new = [], [], []
    for _ in range(args.rounds + 2):
        t_near.append(_time_ms(lambda: wc.nearest(q)))
        t_old.append(_time_ms(old))
        t_new.append(_time_ms(lambda: wc.count(q)))
    wc.close()
    nq = args.n_tally
    med = lambda ts: round(float(np.median(ts[2:])), 3)  # noqa: E731
    return {"nq": nq, "nw": int(wl3.size), "nearest_ms": med(t_near), "nearest_plus_bincount_ms": med(t_old),
            "count_ms": med(t_new), "speedup_vs_nearest_plus_bincount": round(med(t_old) / med(t_new), 3),
            "pcie_bytes_nearest": {"in": nq * 8, "out": nq * 5},
            "pcie_bytes_count": {"in": nq * 8, "out": (int(wl3.size) + 3) * 8}}


def molecules_step(args):
    """MoleculeCounter.update_device, device-resident, against what the library could do before it
    with the same data: DeviceCounter.update_device on precomputed composite keys (8 B/read, 24 B
    slots) plus sct_index_tally on the indices (4 B/read).  Input: config 4's queries against the
    737,280 whitelist answered by the nearest plan (so -1 / -2 are in), and 10-base ThreeBit UMIs
    drawn per barcode from a pool sized for a mean of about four reads per molecule, 1 % with an N.
    Tables are sized up front (the growth is counter_A's subject); both sides alternate within every
    round, per pre-aggregation mode.  Every round is one line of profiles/ab_molecules_<tag>.jsonl."""
    import ctypes

    import numpy as np
    import torch
    from sctools_amd import _lib, counting

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    dev = torch.device("cuda")
    lib = _lib.lib()
    vp = ctypes.c_void_p
    out = {"n": n, "nw": nw, "umi_length": UL, "umi_pool_per_barcode": pool, "capacity_hint": hint, "inputs": {}}

    def run_molecules(mode, d_index, d_umi):
        with _lib.tuning(count_preagg=mode), counting.MoleculeCounter(nw, UL, capacity_hint=hint) as mc:
            def go():
                mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), n)
                torch.cuda.synchronize()
            ms = _time_ms(go)
            reads, molecules, n_none, n_amb, n_bad = mc.counts()
            info = mc.info()
        return ms, (int(reads.sum()), int(molecules.sum()), n_none, n_amb, n_bad, info["nmolecules"], info["capacity"])

    def run_yardstick(mode, d_index, d_keys):
        d_counts = torch.zeros(nw, dtype=torch.int64, device=dev)
        d_tally = torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        with _lib.tuning(count_preagg=mode), counting.DeviceCounter(capacity_hint=hint) as dc:
            def go():
                dc.update_device(d_keys.data_ptr(), n)
                _lib.check(lib.sct_index_tally(vp(d_index.data_ptr()), n, nw, vp(d_counts.data_ptr()),
                                               vp(d_tally.data_ptr()), None))
                torch.cuda.synchronize()
            ms = _time_ms(go)
            nunique = len(dc)
        return ms, nunique

    d_index, d_umi, d_keys = inputs["shuffled"]
    run_molecules(2, d_index, d_umi), run_yardstick(1, d_index, d_keys)  # warm-up: code objects, pool
    facts = None
    lines = []
    for which, (di, du, dk) in inputs.items():
        rounds = []
        for r in range(args.rounds):
            row = {"input": which, "round": r, "n": n, "nw": nw}
            for m, name in MODES.items():
                ms, f = run_molecules(m, di, du)
                assert facts is None or f == facts, (f, facts)  # every mode, order and round: the same numbers
                facts = f
                yms, nunique = run_yardstick(m, di, dk)
                row[name] = {"molecules_ms": round(ms, 3), "counter_plus_tally_ms": round(yms, 3)}
            rounds.append(row)
        lines += rounds
        res = out["inputs"][which] = {}
        for name in MODES.values():
            a = [row[name]["molecules_ms"] for row in rounds]
            b = [row[name]["counter_plus_tally_ms"] for row in rounds]
            med = float(np.median(a))
            res[name] = {
                "molecules_ms": {"median": round(med, 3), "min": min(a), "max": max(a)},
                "counter_plus_tally_ms": {"median": round(float(np.median(b)), 3), "min": min(b), "max": max(b)},
                "bytes_per_read_algorithmic": 12,
                "read_fraction_of_8TBps": round(n * 12 / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
    reads, molecules, n_none, n_amb, n_bad, nmol, cap = facts
    assert reads + n_none + n_amb + n_bad == n and molecules == nmol
    out.update(reads=reads, molecules=molecules, n_none=n_none, n_ambiguous=n_amb, n_bad_umi=n_bad, capacity=cap,
               reads_per_molecule=round(reads / max(1, molecules), 3), yardstick_nunique=nunique)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ab_molecules_%s.jsonl" % args.tag), "w") as f:
        for row in lines:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    return out


def _molecules_input(args):
    """(nw, UMI length, n, capacity hint, UMIs per barcode, {order: (d_index, d_umi, d_keys)}): the
    molecules step's reads, on the device."""
    import numpy as np
    import torch
    from sctools_amd import _lib, synthetic

    nw, L, seed = synthetic.CONFIGS[4]
    UL, n = 10, args.n_a
    wl3 = synthetic.two_to_three(synthetic.whitelist_codes(nw, L, seed), L)
    dev = torch.device("cuda")
    q, _, _ = synthetic.config4_queries(wl3, n, seed=4, device=dev)
    d_wl = torch.from_numpy(wl3.view(np.int64)).cuda()
    d_index = torch.empty(n, dtype=torch.int32, device=dev)
    d_dist = torch.empty(n, dtype=torch.uint8, device=dev)
    plan = _lib.NearestPlan(3, d_wl.data_ptr(), nw, 3 * L, 1)
    plan.query(q.data_ptr(), n, d_index.data_ptr(), d_dist.data_ptr())
    torch.cuda.synchronize()
    plan.close()
    del q, d_dist
    g = torch.Generator(device=dev).manual_seed(7)
    # reads per barcode r = (matched reads) / nw; a pool of r / 4 UMIs per barcode gives ~4 reads per molecule
    matched = int((d_index >= 0).sum())
    pool = max(1, round(matched / nw / 4))
    table = torch.zeros(4096, dtype=torch.int64, device=dev)  # 4096 distinct good UMI codes
    t = torch.randperm(4 ** UL, device=dev, generator=g)[:4096]
    for p in range(UL):
        table |= (((t >> (2 * p)) & 3) + 1) << (3 * p)
    pick = (torch.randint(0, pool, (n,), device=dev, generator=g) + d_index.to(torch.int64) * 31) % 4096
    d_umi = table[pick]
    with_n = torch.rand(n, device=dev, generator=g) < 0.01
    d_umi = torch.where(with_n, d_umi | 6, d_umi)
    d_keys = (d_index.to(torch.int64) << (3 * UL)) | d_umi  # the yardstick's composite keys
    del pick, with_n, t
    torch.cuda.synchronize()
    hint = 1 << max(6, (n // 2).bit_length())  # at most n / 4 molecules expected: load stays below 1/2
    # the same reads in two orders: as drawn (a molecule's reads far apart), and with every molecule's
    # reads adjacent (molecules in hash order) -- the two ends of how close PCR duplicates can lie
    # (an odd multiplier permutes the int64 keys: equal keys stay together, their order is scrambled)
    order = torch.argsort(d_keys * -7046029254386353131)
    inputs = {"shuffled": (d_index, d_umi, d_keys),
              "adjacent": (d_index[order].contiguous(), d_umi[order].contiguous(), d_keys[order].contiguous())}
    del order
    torch.cuda.synchronize()
    return nw, UL, n, hint, pool, inputs


UPDATE_CALLS = ("sct_tune_set", "sct_molecules_create", "sct_molecules_create_counted", "sct_molecules_update",
                "sct_molecules_counts_host", "sct_molecules_destroy")


def _parent_lib(args, names=UPDATE_CALLS):
    """--parent-lib loaded beside this library, with the signatures of the calls in `names`; None without it."""
    import ctypes

    from sctools_amd import _lib
    if not args.parent_lib:
        return None
    old = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in names:
        getattr(old, name).argtypes = _lib.SIGNATURES[name]
    return old


def _full_update(lib, mode, d_index, d_umi, counted, shape):
    """(ms, facts): sct_molecules_update of all n reads into a fresh counter of `lib`, through the C ABI;
    shape = (nw, UL, n, hint)."""
    import ctypes

    import numpy as np
    import torch
    from sctools_amd import _lib
    nw, UL, n, hint = shape
    vp, h = ctypes.c_void_p, ctypes.c_void_p()
    assert lib.sct_tune_set(_lib.TUNE_KEYS["count_preagg"], mode) == 0
    create = lib.sct_molecules_create_counted if counted else lib.sct_molecules_create
    assert create(nw, 3, UL, hint, ctypes.byref(h)) == 0
    try:
        def go():
            assert lib.sct_molecules_update(h, vp(d_index.data_ptr()), vp(d_umi.data_ptr()), n, None) == 0
            torch.cuda.synchronize()
        ms = _time_ms(go)
        reads, molecules, tally = np.empty(nw, np.uint64), np.empty(nw, np.uint64), np.empty(3, np.uint64)
        assert lib.sct_molecules_counts_host(h, _lib._ptr(reads), _lib._ptr(molecules), _lib._ptr(tally)) == 0
    finally:
        lib.sct_molecules_destroy(h)
        lib.sct_tune_set(_lib.TUNE_KEYS["count_preagg"], -1)
    return ms, (int(reads.sum()), int(molecules.sum()), int(tally[0]), int(tally[1]), int(tally[2]))


def _vs_parent(a, b):
    """This library's {median, min, max} beside the parent's: they agree when the medians differ by no
    more than the min-max spread of the parent's own rounds."""
    return {"median_difference_ms": round(a["median"] - b["median"], 3),
            "parent_spread_ms": round(b["max"] - b["min"], 3),
            "agree": abs(a["median"] - b["median"]) <= b["max"] - b["min"]}


def _features_of(d_index, d_umi, spread, nf):
    """A molecule's feature: a hash of its (barcode, UMI) over `spread` of the nf features, 2 % none."""
    import torch
    g = torch.Generator(device=d_index.device).manual_seed(13)
    f = (((d_umi * -7046029254386353131) >> 40) ^ d_index.to(torch.int64)) & (spread - 1)
    f = (f * (nf // spread)).to(torch.int32)  # spread over the whole range of nf
    none = torch.rand(d_index.numel(), device=d_index.device, generator=g) < 0.02
    return torch.where(none, torch.full_like(f, -1), f).contiguous()


def collapse_step(args):
    """The counted molecule counter and its UMI collapse on the molecules step's input.  Alternating
    within every round, per input order and pre-aggregation mode: (a) MoleculeCounter.update_device as
    it was (no read counts), (a') the same call into the library given by --parent-lib (the commit
    before the counted counter, loaded beside this one; skipped without it), (b) update_device with
    read_counts=True, (c) collapse_device on the table (b) left, one lane per slot and then a wave per
    molecule (SCT_TUNE_COLLAPSE_FORM 0 / 1, the default).  Then, once, the host way to (c)'s
    answer: pairs(reads=True) to the host, and a Python dict collapse of the first --n-collapse-host
    molecules (whole barcodes), scaled by molecules / sub-sample; its collapsed counts must equal the
    device's for those barcodes.  (a) and (a') agree when their medians differ by no more than the
    min-max spread of (a')'s own rounds; the step fails when they do not.  Every round is one line of
    profiles/ab_umi_collapse_<tag>.jsonl, the summary its last."""
    import numpy as np
    import torch
    from sctools_amd import _lib, counting

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    dev = torch.device("cuda")
    # (a library from before the counted counter will do: only the plain update is asked of it)
    old = _parent_lib(args, [name for name in UPDATE_CALLS if name != "sct_molecules_create_counted"])
    d_collapsed = torch.zeros(nw + 1, dtype=torch.int64, device=dev)

    def facts_of(reads, molecules, tally):
        return int(reads.sum()), int(molecules.sum()), int(tally[0]), int(tally[1]), int(tally[2])

    def run_update(mode, d_index, d_umi, counted):
        """(update ms, collapse ms per SCT_TUNE_COLLAPSE_FORM or None, facts)"""
        mc = counting.MoleculeCounter(nw, UL, capacity_hint=hint, read_counts=counted)
        with _lib.tuning(count_preagg=mode), mc:
            def go():
                mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), n)
                torch.cuda.synchronize()
            ms = _time_ms(go)
            cms = None
            if counted:
                def collapse():
                    mc.collapse_device(d_collapsed.data_ptr(), d_collapsed.data_ptr() + 8 * nw)
                    torch.cuda.synchronize()
                cms = []
                for form in (0, 1):
                    with _lib.tuning(collapse_form=form):
                        cms.append(_time_ms(collapse))
            reads, molecules, n_none, n_amb, n_bad = mc.counts()
        return ms, cms, facts_of(reads, molecules, (n_none, n_amb, n_bad))

    def run_parent(mode, d_index, d_umi):
        return _full_update(old, mode, d_index, d_umi, False, (nw, UL, n, hint))

    run_update(2, *inputs["shuffled"][:2], True)  # warm-up: code objects, pool
    if old:
        run_parent(2, *inputs["shuffled"][:2])
    facts, lines = None, []
    out = {"n": n, "nw": nw, "umi_length": UL, "umi_pool_per_barcode": pool, "capacity_hint": hint, "inputs": {},
           "parent_lib": bool(old)}
    for which, (di, du, _) in inputs.items():
        rounds = []
        for r in range(args.rounds):
            row = {"input": which, "round": r, "n": n, "nw": nw}
            for m, name in MODES.items():
                cell = {}
                ms, _, f = run_update(m, di, du, False)
                cell["uncounted_ms"] = round(ms, 3)
                assert facts is None or f == facts, (f, facts)  # every library, form, order and round: the same numbers
                facts = f
                if old:
                    ms, f = run_parent(m, di, du)
                    cell["uncounted_parent_ms"] = round(ms, 3)
                    assert f == facts, (f, facts)
                ms, cms, f = run_update(m, di, du, True)
                cell["counted_ms"] = round(ms, 3)
                cell["collapse_lane_ms"], cell["collapse_wave_ms"] = round(cms[0], 3), round(cms[1], 3)
                assert f == facts, (f, facts)
                row[name] = cell
            rounds.append(row)
        lines += rounds
        res = out["inputs"][which] = {}
        for name in MODES.values():
            res[name] = {}
            for key in rounds[0][name]:
                a = [row[name][key] for row in rounds]
                res[name][key] = {"median": round(float(np.median(a)), 3), "min": min(a), "max": max(a)}
            if old:
                res[name]["uncounted_vs_parent"] = _vs_parent(res[name]["uncounted_ms"], res[name]["uncounted_parent_ms"])
    # (d) the host way: the counted rows to the host, and a dict collapse of a prefix of whole barcodes
    di, du, _ = inputs["shuffled"]
    with counting.MoleculeCounter(nw, UL, capacity_hint=hint, read_counts=True) as mc:
        mc.update_device(di.data_ptr(), du.data_ptr(), n)
        got = {}
        fetch_ms = _time_ms(lambda: got.update(rows=mc.pairs(reads=True)))
        collapsed, n_corrected = mc.collapse()
        index, umi, mreads = got["rows"]
    nmol = int(index.size)
    k = min(nmol, args.n_collapse_host)
    if k < nmol:
        k = int(np.searchsorted(index, index[k], side="left"))  # whole barcodes only
    sub_i, sub_u, sub_r = index[:k].tolist(), umi[:k].tolist(), mreads[:k].tolist()

    def host_collapse():
        table = {(i << (3 * UL)) | u: r for i, u, r in zip(sub_i, sub_u, sub_r)}
        images, moved = set(), 0
        for key, r in table.items():
            best, best_r = key, r
            for p in range(UL):
                t = (key >> (3 * p)) & 7
                for b in (1, 2, 3, 4):
                    if b != t:
                        v = key ^ ((t ^ b) << (3 * p))
                        vr = table.get(v)
                        if vr is not None and (vr, v) > (best_r, best):
                            best, best_r = v, vr
            images.add(best)
            moved += best != key
        return np.bincount(np.array([v >> (3 * UL) for v in images], dtype=np.int64), minlength=nw), moved

    host = {}
    dict_ms = _time_ms(lambda: host.update(res=host_collapse()))
    nb = int(index[k - 1]) + 1 if k else 0
    assert np.array_equal(host["res"][0][:nb], collapsed[:nb]), "the device's collapse differs from the host's"
    scale = nmol / max(1, k)
    coll = [row[name]["collapse_lane_ms"] for row in lines for name in MODES.values()]
    wave = [row[name]["collapse_wave_ms"] for row in lines for name in MODES.values()]
    out["host_yardstick"] = {"fetch_counted_host_ms": round(fetch_ms, 1), "dict_collapse_molecules": k,
                             "dict_collapse_ms": round(dict_ms, 1), "scale": round(scale, 2),
                             "dict_collapse_scaled_ms": round(dict_ms * scale, 1),
                             "total_scaled_ms": round(fetch_ms + dict_ms * scale, 1),
                             "n_corrected_in_sub_sample": int(host["res"][1])}
    out["collapse_lane_ms"] = {"median": round(float(np.median(coll)), 3), "min": min(coll), "max": max(coll)}
    out["collapse_wave_ms"] = {"median": round(float(np.median(wave)), 3), "min": min(wave), "max": max(wave)}
    reads, molecules, n_none, n_amb, n_bad = facts
    assert reads + n_none + n_amb + n_bad == n and molecules == nmol
    out.update(reads=reads, molecules=molecules, collapsed=int(collapsed.sum()), n_corrected=n_corrected,
               n_none=n_none, n_ambiguous=n_amb, n_bad_umi=n_bad,
               collapse_ns_per_molecule=round(out["collapse_wave_ms"]["median"] * 1e6 / max(1, nmol), 3))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ab_umi_collapse_%s.jsonl" % args.tag), "w") as f:
        for row in lines:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    # the plain update must be the earlier library's: the step fails (its profile is written) if not
    apart = ["%s/%s: %s" % (which, name, v["uncounted_vs_parent"]) for which, modes in out["inputs"].items()
             for name, v in modes.items() if old and not v["uncounted_vs_parent"]["agree"]]
    assert not apart, "the plain update differs from --parent-lib beyond that library's own spread: " + "; ".join(apart)
    return out


def merge_step(args):
    """MoleculeCounter.merge on the molecules step's input (as drawn) split in two halves by read
    position, so that molecules straddle the halves: `a` holds the first half, `b` the second, tables
    sized up front so that nothing grows.  Alternating within every round, plain and counted: (m) the
    merge of b into a fresh a, the table read in place; (d) the same merge with b's rows compacted and
    copied first (SCT_TUNE_MERGE_ROWS 1, the route between two devices, here on one); (x) with two
    devices visible, b on the second device; (y) the yardstick: sct_molecules_update, form 0, into a
    fresh a of as many reads as b has molecules -- b's molecules once each in random order, the same
    claims on the same table.  Then, once, the host route of today: b.pairs(reads=True) to the host and
    every row replayed mreads times through update.  Then the existing rows of the molecules and
    collapse steps again (the plain and the counted update of all reads, both orders, the three
    forms) in this library and, alternating, in --parent-lib; they agree when the medians differ by
    no more than the parent's own min-max spread, and the step fails (its profile written) when not.
    Every round is one line of profiles/ab_molecules_merge_<tag>.jsonl, the summary its last."""
    import numpy as np
    import torch
    from sctools_amd import _lib, counting

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    dev = torch.device("cuda")
    di, du, _ = inputs["shuffled"]
    half = n // 2
    halves = [(di[:half], du[:half]), (di[half:], du[half:])]
    two_devices = _lib.device_count() >= 2

    def fed(part, counted, capacity, device=None):
        mc = counting.MoleculeCounter(nw, UL, capacity_hint=capacity, read_counts=counted, device=device)
        i, u = halves[part]
        if device not in (None, 0):
            with torch.cuda.device(device):
                i, u = i.to("cuda:%d" % device), u.to("cuda:%d" % device)
                mc.update_device(i.data_ptr(), u.data_ptr(), i.numel())
                torch.cuda.synchronize()
        else:
            mc.update_device(i.data_ptr(), u.data_ptr(), i.numel())
        torch.cuda.synchronize()
        return mc

    def facts_of(mc):
        reads, molecules, n_none, n_amb, n_bad = mc.counts()
        info = mc.info()
        return int(reads.sum()), int(molecules.sum()), n_none, n_amb, n_bad, info["nmolecules"], info["total"]

    out = {"n": n, "nw": nw, "umi_length": UL, "two_devices": two_devices, "parent_lib": bool(args.parent_lib)}
    lines, whole = [], None
    for counted in (False, True):
        name = "counted" if counted else "plain"
        b = fed(1, counted, hint)
        nb = len(b)
        probe = fed(0, counted, hint)
        na = len(probe)
        probe.close()
        cap = 64
        while cap // 2 < na + nb:
            cap *= 2
        # the yardstick's reads: b's molecules, once each, in random order
        y_index = torch.empty(nb, dtype=torch.int32, device=dev)
        y_umi = torch.empty(nb, dtype=torch.int64, device=dev)
        b.fetch_device(y_index.data_ptr(), y_umi.data_ptr(), nb)
        torch.cuda.synchronize()
        perm = torch.randperm(nb, device=dev, generator=torch.Generator(device=dev).manual_seed(11))
        y_index, y_umi = y_index[perm].contiguous(), y_umi[perm].contiguous()
        del perm
        b_far = fed(1, counted, hint, device=1) if two_devices else None
        torch.cuda.synchronize()

        def timed_merge(src, rows):
            a = fed(0, counted, cap)
            with _lib.tuning(merge_rows=rows), a:
                def go():
                    a.merge_device(src)
                    torch.cuda.synchronize()
                ms = _time_ms(go)
                f = facts_of(a)
                assert a.info()["capacity"] == cap  # sized up front: the merge did not grow it
            return ms, f

        def timed_yardstick():
            a = fed(0, counted, cap)
            with _lib.tuning(count_preagg=0), a:
                def go():
                    a.update_device(y_index.data_ptr(), y_umi.data_ptr(), nb)
                    torch.cuda.synchronize()
                ms = _time_ms(go)
                nmol = len(a)
            return ms, nmol

        timed_merge(b, 0), timed_merge(b, 1), timed_yardstick()  # warm-up: code objects, pool
        rounds = []
        for r in range(args.rounds):
            row = {"what": name, "round": r, "n": n, "src_molecules": nb, "dst_molecules": na, "dst_capacity": cap}
            ms, f = timed_merge(b, 0)
            assert whole is None or f == whole, (f, whole)  # every route, form and round: the same numbers
            whole = f
            row["merge_ms"] = round(ms, 3)
            ms, f = timed_merge(b, 1)
            assert f == whole, (f, whole)
            row["merge_compacted_ms"] = round(ms, 3)
            if b_far is not None:
                ms, f = timed_merge(b_far, 0)
                assert f == whole, (f, whole)
                row["merge_other_device_ms"] = round(ms, 3)
            ms, nmol = timed_yardstick()
            assert nmol == whole[5], (nmol, whole)
            row["update_form0_src_molecules_ms"] = round(ms, 3)
            rounds.append(row)
        lines += rounds
        res = out[name] = {"src_molecules": nb, "dst_molecules": na, "merged_molecules": whole[5],
                           "dst_capacity": cap, "src_capacity": b.info()["capacity"]}
        for key in rounds[0]:
            if key.endswith("_ms"):
                v = [row[key] for row in rounds]
                res[key] = {"median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
        res["merge_over_yardstick"] = round(res["merge_ms"]["median"] / res["update_form0_src_molecules_ms"]["median"], 3)
        res["merge_ns_per_src_molecule"] = round(res["merge_ms"]["median"] * 1e6 / nb, 3)
        if counted:  # the host route a user has today (it loses b's tallies; the molecules and reads are right)
            a = fed(0, True, cap)
            got = {}
            fetch_ms = _time_ms(lambda: got.update(rows=b.pairs(reads=True)))
            index, umi, mreads = got["rows"]

            def replay():
                a.update(np.repeat(index, mreads), np.repeat(umi, mreads))
            replay_ms = _time_ms(replay)
            assert len(a) == whole[5]
            a.close()
            out["host_route"] = {"pairs_reads_ms": round(fetch_ms, 1), "repeat_and_update_ms": round(replay_ms, 1),
                                 "total_ms": round(fetch_ms + replay_ms, 1), "reads_replayed": int(mreads.sum())}
            del index, umi, mreads, got
        if b_far is not None:
            b_far.close()
        b.close()
        del y_index, y_umi
    reads, molecules, n_none, n_amb, n_bad, nmol, total = whole
    assert total == n and reads + n_none + n_amb + n_bad == n and molecules == nmol
    out.update(reads=reads, molecules=molecules, n_none=n_none, n_ambiguous=n_amb, n_bad_umi=n_bad)

    # the existing rows again, this library and the parent's alternating
    old = _parent_lib(args)
    full_update = functools.partial(_full_update, shape=(nw, UL, n, hint))
    libs = {"this": _lib.lib()}
    if old:
        libs["parent"] = old
    out["existing_rows"] = {}
    for which, (xi, xu, _) in inputs.items():
        full_update(_lib.lib(), 1, xi, xu, True)
        rounds = []
        for r in range(args.rounds):
            row = {"what": "existing", "input": which, "round": r}
            for m, mname in MODES.items():
                cell = {}
                for counted in (False, True):
                    for lname, lib in libs.items():
                        ms, f = full_update(lib, m, xi, xu, counted)
                        assert f == whole[:5], (f, whole)
                        cell["%s_%s_ms" % ("counted" if counted else "plain", lname)] = round(ms, 3)
                row[mname] = cell
            rounds.append(row)
        lines += rounds
        res = out["existing_rows"][which] = {}
        for mname in MODES.values():
            res[mname] = {}
            for key in rounds[0][mname]:
                v = [row[mname][key] for row in rounds]
                res[mname][key] = {"median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
            for kind in ("plain", "counted") if old else ():
                res[mname][kind + "_vs_parent"] = _vs_parent(res[mname][kind + "_this_ms"], res[mname][kind + "_parent_ms"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ab_molecules_merge_%s.jsonl" % args.tag), "w") as f:
        for row in lines:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    apart = ["%s/%s/%s: %s" % (which, mname, kind, v[kind + "_vs_parent"])
             for which, modes in out["existing_rows"].items() for mname, v in modes.items()
             for kind in ("plain", "counted") if old and not v[kind + "_vs_parent"]["agree"]]
    assert not apart, "an update differs from --parent-lib beyond that library's own spread: " + "; ".join(apart)
    return out


def matrix_step(args):
    """The count matrix on the molecules step's input with a feature column: nf = 4096, ThreeBit, a
    molecule's feature a hash of its (barcode, UMI) so that the molecules are the plain run's, 2 % of
    the reads with no feature; `spread` of the 4,096 features are in use (4096: about as many entries
    as molecules, a gene-like matrix; 16: a tag panel, many molecules per entry).  Alternating within
    every round, per input order and pre-aggregation mode: the plain update (12 B/read) in this
    library and in --parent-lib, the counted one likewise, and update_features (16 B/read) plain and
    counted.  Then per spread, on the table the counted feature update left: matrix_device with the
    molecules only, with reads, and with reads and collapsed, all outputs device-resident; and once the
    host route, pairs(features=True) to the host and np.unique over (barcode, feature).  The plain and
    the counted update agree with the parent when the medians differ by no more than the min-max
    spread of the parent's own rounds; the step fails (its profile written) when they do not.  Every
    round is one line of the profile, the summary its last."""
    import numpy as np
    import torch
    from sctools_amd import _lib, counting

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    nf = 4096
    dev = torch.device("cuda")
    old = _parent_lib(args)
    full_update = functools.partial(_full_update, shape=(nw, UL, n, hint))

    features_of = functools.partial(_features_of, nf=nf)

    def feature_update(mode, d_index, d_feature, d_umi, counted, keep=False):
        mc = counting.MoleculeCounter(nw, UL, capacity_hint=hint, read_counts=counted, features=nf)
        with _lib.tuning(count_preagg=mode):
            def go():
                mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), n, feature_ptr=d_feature.data_ptr())
                torch.cuda.synchronize()
            ms = _time_ms(go)
        reads, molecules, n_none, n_amb, n_bad = mc.counts()
        f = (int(reads.sum()) + mc.n_no_feature, int(molecules.sum()), n_none, n_amb, n_bad)
        if keep:
            return ms, f, mc
        mc.close()
        return ms, f

    libs = {"this": _lib.lib()}
    if old:
        libs["parent"] = old
    out = {"n": n, "nw": nw, "nf": nf, "umi_length": UL, "capacity_hint": hint, "parent_lib": bool(old),
           "bytes_per_read": {"plain": 12, "features": 16}, "updates": {}, "matrix": {}}
    lines, facts = [], None
    feats = {which: features_of(di, du, nf) for which, (di, du, _) in inputs.items()}
    for which, (di, du, _) in inputs.items():
        df = feats[which]
        full_update(_lib.lib(), 1, di, du, True), feature_update(1, di, df, du, True)  # warm-up
        rounds = []
        for r in range(args.rounds):
            row = {"what": "update", "input": which, "round": r}
            for m, mname in MODES.items():
                cell = {}
                for counted in (False, True):
                    kind = "counted" if counted else "plain"
                    for lname, lib in libs.items():
                        ms, f = full_update(lib, m, di, du, counted)
                        assert facts is None or f == facts, (f, facts)
                        facts = f
                        cell["%s_%s_ms" % (kind, lname)] = round(ms, 3)
                    ms, f = feature_update(m, di, df, du, counted)
                    # the reads without a feature are the only ones the plain run counted and this one did not
                    assert f[0] == facts[0] and f[2:] == facts[2:], (f, facts)
                    cell["%s_features_ms" % kind] = round(ms, 3)
                row[mname] = cell
            rounds.append(row)
        lines += rounds
        res = out["updates"][which] = {}
        for mname in MODES.values():
            res[mname] = {}
            for key in rounds[0][mname]:
                v = [row[mname][key] for row in rounds]
                res[mname][key] = {"median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
            for kind in ("plain", "counted"):
                a = res[mname][kind + "_this_ms"]
                res[mname][kind + "_features_over_plain"] = round(res[mname][kind + "_features_ms"]["median"] / a["median"], 3)
                if old:
                    res[mname][kind + "_vs_parent"] = _vs_parent(a, res[mname][kind + "_parent_ms"])
    # the matrix, per spread of the features, on the reads as drawn
    di, du, _ = inputs["shuffled"]
    for spread in (nf, 16):
        df = features_of(di, du, spread)
        _, _, mc = feature_update(1, di, df, du, True, keep=True)
        nmol = len(mc)
        o_indptr = torch.empty(nw + 1, dtype=torch.int64, device=dev)
        o_feat = torch.empty(nmol, dtype=torch.int32, device=dev)
        o_val = torch.empty((3, nmol), dtype=torch.int64, device=dev)
        forms = {"molecules": (o_val[0].data_ptr(), None, None),
                 "molecules_reads": (o_val[0].data_ptr(), o_val[1].data_ptr(), None),
                 "molecules_reads_collapsed": (o_val[0].data_ptr(), o_val[1].data_ptr(), o_val[2].data_ptr())}
        got = {}

        def run_matrix(form):
            def go():
                got["nnz"] = mc.matrix_device(o_indptr.data_ptr(), o_feat.data_ptr(), *forms[form], nmol)
                torch.cuda.synchronize()
            return _time_ms(go)

        d_collapsed = torch.empty(nw + 1, dtype=torch.int64, device=dev)

        def run_collapse():
            def go():
                mc.collapse_device(d_collapsed.data_ptr(), d_collapsed.data_ptr() + 8 * nw)
                torch.cuda.synchronize()
            return _time_ms(go)

        run_matrix("molecules_reads_collapsed")  # warm-up
        rounds = []
        for r in range(args.rounds):
            row = {"what": "matrix", "spread": spread, "round": r}
            for form in forms:
                row[form + "_ms"] = round(run_matrix(form), 3)
            row["collapse_alone_ms"] = round(run_collapse(), 3)
            rounds.append(row)
        lines += rounds
        nnz = got["nnz"]
        res = out["matrix"]["spread_%d" % spread] = {"molecules": nmol, "nnz": nnz}
        for key in rounds[0]:
            if key.endswith("_ms"):
                v = [row[key] for row in rounds]
                res[key] = {"median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
        # the host route: the rows to the host, np.unique over (barcode, feature)
        rows = {}
        pairs_ms = _time_ms(lambda: rows.update(r=mc.pairs(features=True, reads=True)))
        pi, pf, pu, pr = rows["r"]

        def group():
            cell = pi.astype(np.int64) * nf + pf
            uniq, start, count = np.unique(cell, return_index=True, return_counts=True)
            rows["m"] = (uniq, count, np.add.reduceat(pr, start))
        unique_ms = _time_ms(group)
        uniq, count, rsum = rows["m"]
        full = mc.matrix(reads=True, collapsed=True)
        assert full[1].size == nnz == uniq.size and np.array_equal(uniq % nf, full[1])
        assert np.array_equal(count, full[2]) and np.array_equal(rsum, full[3])
        collapsed, _ = mc.collapse()
        assert int(full[4].sum()) == int(collapsed.sum()) and int(full[2].sum()) == nmol
        res["host_route"] = {"pairs_features_reads_ms": round(pairs_ms, 1), "np_unique_ms": round(unique_ms, 1),
                             "total_ms": round(pairs_ms + unique_ms, 1)}
        res["matrix_host_ms"] = round(_time_ms(lambda: mc.matrix(reads=True, collapsed=True)), 1)
        res["host_route_over_matrix_device"] = round((pairs_ms + unique_ms) / res["molecules_reads_ms"]["median"], 1)
        mc.close()
        del o_indptr, o_feat, o_val, rows, pi, pf, pu, pr, full, df
    out["matrix_device_ms"] = {k: v["molecules_reads_collapsed_ms"]["median"] for k, v in out["matrix"].items()}
    reads, molecules, n_none, n_amb, n_bad = facts
    out.update(reads=reads, n_none=n_none, n_ambiguous=n_amb, n_bad_umi=n_bad)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = "ab_count_matrix.jsonl" if args.tag == "run" else "ab_count_matrix_%s.jsonl" % args.tag
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        for row in lines:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    apart = ["%s/%s/%s: %s" % (which, mname, kind, v[kind + "_vs_parent"])
             for which, modes in out["updates"].items() for mname, v in modes.items()
             for kind in ("plain", "counted") if old and not v[kind + "_vs_parent"]["agree"]]
    assert not apart, "an update differs from --parent-lib beyond that library's own spread: " + "; ".join(apart)
    return out


CALLS_ABI = UPDATE_CALLS + (
    "sct_molecules_create_features", "sct_molecules_update_features", "sct_molecules_info", "sct_molecules_fetch",
    "sct_molecules_fetch_counted", "sct_molecules_fetch_features", "sct_molecules_collapse", "sct_molecules_matrix",
    "sct_molecules_merge", "sct_counter_create", "sct_counter_update", "sct_counter_info", "sct_counter_fetch",
    "sct_counter_destroy")
# the calls step's calls that an earlier library may lack: {call: the symbol it needs}
CALLS_NEWER = {"collapse_directional": "sct_molecules_collapse_by", "downsample_half": "sct_molecules_downsample",
               "downsample_curve_k16": "sct_molecules_downsample_curve"}


def calls_step(args):
    """The calls that read a table back, merge two and grow one, in this library and in --parent-lib
    (without it: this library alone, nothing compared), through the C ABI with device-resident outputs
    and a stream synchronise inside the timed window.  On the molecules step's input as drawn, per
    library, filled once: a counted feature counter (nf = 4096), a counted plain counter and a barcode
    counter of the composite keys.  Timed, alternating between the libraries within every round (each
    goes first in every other round, and every timed call follows an untimed one of its own kind):
    sct_molecules_fetch; sct_molecules_fetch_counted without and with parents;
    sct_molecules_fetch_features with every column; sct_molecules_collapse; sct_molecules_matrix with
    the molecules, with reads, with reads and collapsed; sct_molecules_collapse_by with
    SCT_COLLAPSE_DIRECTIONAL; sct_molecules_merge of the plain counter into an empty counter sized up
    front, the table in place and compacted first (SCT_TUNE_MERGE_ROWS 1); sct_molecules_downsample of
    it at threshold 2^31 into such a counter; sct_molecules_downsample_curve at 16 points;
    sct_molecules_update of all reads into a counter sized up front and from capacity_hint 0 (the
    growth path), plain and counted; sct_counter_fetch.  A call whose symbol --parent-lib lacks is timed
    in this library alone.  Before the rounds every call runs once in each library and every output
    array must be equal element for element.  A call agrees when the medians differ by no more than
    the min-max spread of the parent's own rounds; the step fails (its profile written) when a call is
    slower than the parent beyond that spread; one that is faster beyond it is reported.  Every round
    is one line of profiles/ab_molecules_calls_<tag>.jsonl, the summary its last."""
    import ctypes

    import numpy as np
    import torch
    from sctools_amd import _lib

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    nf = 4096
    di, du, dk = inputs["shuffled"]
    df = _features_of(di, du, nf, nf)
    dev = torch.device("cuda")
    vp, i64, ref = ctypes.c_void_p, ctypes.c_int64, ctypes.byref
    libs = {"this": _lib.lib()}
    old = _parent_lib(args, CALLS_ABI)
    lacking = set()  # the calls the parent library has no symbol for
    if old:
        libs["parent"] = old
        for name, symbol in CALLS_NEWER.items():
            if hasattr(old, symbol):
                getattr(old, symbol).argtypes = _lib.SIGNATURES[symbol]
            else:
                lacking.add(name)
    ptr = lambda t: vp(t.data_ptr())  # noqa: E731
    points = np.array([((t + 1) << 32) // 16 for t in range(16)], dtype=np.uint64)  # the curve's thresholds

    class Side:
        """One library's counters and output arrays."""
        def __init__(self, lib):
            self.lib = lib
            self.feat, self.plain, self.counter = vp(), vp(), vp()
            assert lib.sct_molecules_create_features(nw, nf, 3, UL, hint, 1, -1, ref(self.feat)) == 0
            assert lib.sct_molecules_update_features(self.feat, ptr(di), ptr(df), ptr(du), n, None) == 0
            assert lib.sct_molecules_create_counted(nw, 3, UL, hint, ref(self.plain)) == 0
            assert lib.sct_molecules_update(self.plain, ptr(di), ptr(du), n, None) == 0
            assert lib.sct_counter_create(hint, ref(self.counter)) == 0
            assert lib.sct_counter_update(self.counter, ptr(dk), n, None) == 0
            torch.cuda.synchronize()
            self.nfeat, self.nplain, self.ncodes = self.size(self.feat), self.size(self.plain), i64(0)
            assert lib.sct_counter_info(self.counter, ref(self.ncodes), None, None) == 0
            self.ncodes = self.ncodes.value
            rows = max(self.nfeat, self.nplain, self.ncodes, nw + 1)
            self.i32 = torch.zeros((2, rows), dtype=torch.int32, device=dev)
            self.i64 = torch.zeros((4, rows), dtype=torch.int64, device=dev)
            self.cap = 64
            while self.cap // 2 < self.nplain:
                self.cap *= 2
            self.made = None  # the counter a merge or an update made, kept until its rows are compared

        def size(self, h):
            v = i64(0)
            assert self.lib.sct_molecules_info(h, ref(v), None, None) == 0
            return v.value

        def drop(self):
            if self.made is not None:
                self.lib.sct_molecules_destroy(self.made)
                self.made = None

        def close(self):
            self.drop()
            self.lib.sct_molecules_destroy(self.feat), self.lib.sct_molecules_destroy(self.plain)
            self.lib.sct_counter_destroy(self.counter)

    def timed(call):
        def go():
            assert call() == 0
            torch.cuda.synchronize()
        return _time_ms(go)

    def rows_of(s, h):
        """A made counter's table as arrays: its counted (or plain) rows, reads, molecules and tally."""
        m = s.size(h)
        if counted_of[h.value]:
            assert s.lib.sct_molecules_fetch_counted(h, ptr(s.i32[0]), ptr(s.i64[0]), ptr(s.i64[1]), None, m, None) == 0
        else:
            assert s.lib.sct_molecules_fetch(h, ptr(s.i32[0]), ptr(s.i64[0]), m, None) == 0
        torch.cuda.synchronize()
        reads, molecules, tally = np.empty(nw, np.uint64), np.empty(nw, np.uint64), np.empty(3, np.uint64)
        assert s.lib.sct_molecules_counts_host(h, _lib._ptr(reads), _lib._ptr(molecules), _lib._ptr(tally)) == 0
        return [s.i32[0, :m].clone(), s.i64[:2, :m].clone() if counted_of[h.value] else s.i64[0, :m].clone(),
                torch.from_numpy(np.concatenate([reads, molecules, tally]).view(np.int64))]

    counted_of = {}

    def make(s, counted, capacity):
        s.drop()
        h = vp()
        create = s.lib.sct_molecules_create_counted if counted else s.lib.sct_molecules_create
        assert create(nw, 3, UL, capacity, ref(h)) == 0
        counted_of[h.value] = counted
        s.made = h
        return h

    def fetch(s):
        ms = timed(lambda: s.lib.sct_molecules_fetch(s.plain, ptr(s.i32[0]), ptr(s.i64[0]), s.nplain, None))
        return ms, [s.i32[0, :s.nplain], s.i64[0, :s.nplain]]

    def fetch_counted(s, parents):
        par = ptr(s.i64[2]) if parents else None
        ms = timed(lambda: s.lib.sct_molecules_fetch_counted(s.plain, ptr(s.i32[0]), ptr(s.i64[0]), ptr(s.i64[1]), par,
                                                             s.nplain, None))
        return ms, [s.i32[0, :s.nplain], s.i64[:3 if parents else 2, :s.nplain]]

    def fetch_features(s):
        ms = timed(lambda: s.lib.sct_molecules_fetch_features(s.feat, ptr(s.i32[0]), ptr(s.i32[1]), ptr(s.i64[0]),
                                                              ptr(s.i64[1]), ptr(s.i64[2]), s.nfeat, None))
        return ms, [s.i32[:, :s.nfeat], s.i64[:3, :s.nfeat]]

    def collapse(s):
        ms = timed(lambda: s.lib.sct_molecules_collapse(s.plain, ptr(s.i64[0]), ptr(s.i64[1]), None))
        return ms, [s.i64[0, :nw], s.i64[1, :1]]

    def matrix(s, values):
        nnz = i64(0)
        val = [ptr(s.i64[1 + k]) if k < values else None for k in range(3)]
        ms = timed(lambda: s.lib.sct_molecules_matrix(s.feat, ptr(s.i64[0]), ptr(s.i32[0]), val[0], val[1], val[2],
                                                      s.nfeat, ref(nnz), None))
        return ms, [s.i64[0, :nw + 1], s.i32[0, :nnz.value], s.i64[1:1 + values, :nnz.value]]

    def merge(s, rows):
        h = make(s, True, s.cap)
        assert s.lib.sct_tune_set(_lib.TUNE_KEYS["merge_rows"], rows) == 0
        try:
            ms = timed(lambda: s.lib.sct_molecules_merge(h, s.plain, None))
        finally:
            s.lib.sct_tune_set(_lib.TUNE_KEYS["merge_rows"], -1)
        return ms, functools.partial(rows_of, s, h)

    def collapse_directional(s):
        ms = timed(lambda: s.lib.sct_molecules_collapse_by(s.plain, _lib.COLLAPSE_DIRECTIONAL, ptr(s.i64[0]),
                                                           ptr(s.i64[1]), None))
        return ms, [s.i64[0, :nw], s.i64[1, :1]]

    def downsample_half(s):
        h = make(s, True, s.cap)
        ms = timed(lambda: s.lib.sct_molecules_downsample(h, s.plain, 1 << 31, 7, None))
        return ms, functools.partial(rows_of, s, h)

    def downsample_curve(s):
        ms = timed(lambda: s.lib.sct_molecules_downsample_curve(s.plain, _lib._ptr(points), points.size, 7,
                                                                ptr(s.i64[0]), ptr(s.i64[1]), None))
        return ms, [s.i64[:2, :points.size]]

    def update(s, counted, capacity=0):
        h = make(s, counted, capacity)
        ms = timed(lambda: s.lib.sct_molecules_update(h, ptr(di), ptr(du), n, None))
        return ms, functools.partial(rows_of, s, h)

    def counter_fetch(s):
        ms = timed(lambda: s.lib.sct_counter_fetch(s.counter, ptr(s.i64[0]), ptr(s.i64[1]), ptr(s.i64[2]), s.ncodes,
                                                   None))
        return ms, [s.i64[:3, :s.ncodes]]

    calls = {"fetch": fetch, "fetch_counted": functools.partial(fetch_counted, parents=False),
             "fetch_counted_parents": functools.partial(fetch_counted, parents=True), "fetch_features": fetch_features,
             "collapse": collapse, "collapse_directional": collapse_directional,
             "matrix_molecules": functools.partial(matrix, values=1),
             "matrix_molecules_reads": functools.partial(matrix, values=2),
             "matrix_molecules_reads_collapsed": functools.partial(matrix, values=3),
             "merge": functools.partial(merge, rows=0), "merge_compacted": functools.partial(merge, rows=1),
             "downsample_half": downsample_half, "downsample_curve_k16": downsample_curve,
             "update": functools.partial(update, counted=False, capacity=hint),
             "update_counted": functools.partial(update, counted=True, capacity=hint),
             "update_growing": functools.partial(update, counted=False),
             "update_growing_counted": functools.partial(update, counted=True), "counter_fetch": counter_fetch}
    sides = {name: Side(lib) for name, lib in libs.items()}
    out = {"n": n, "nw": nw, "nf": nf, "umi_length": UL, "capacity_hint": hint, "parent_lib": bool(old),
           "molecules": sides["this"].nplain, "feature_molecules": sides["this"].nfeat, "codes": sides["this"].ncodes,
           "parent_lacks": sorted(lacking), "outputs_equal": {}, "calls": {}}
    sides_of = {name: [(lname, s) for lname, s in sides.items() if lname == "this" or name not in lacking]
                for name in calls}
    # every call once in each library (the warm-up as well): the outputs, element for element
    for name, call in calls.items():
        got = {}
        for lname, s in sides_of[name]:
            arrays = call(s)[1]
            got[lname] = [a.clone() for a in (arrays() if callable(arrays) else arrays)]
        if "parent" in got:
            same = len(got["this"]) == len(got["parent"]) and all(
                a.shape == b.shape and bool((a == b).all()) for a, b in zip(got["this"], got["parent"]))
            out["outputs_equal"][name] = same
        del got
    lines = []
    for r in range(args.rounds):
        row = {"round": r}
        for name, call in calls.items():
            row[name] = {}
            for lname, s in sides_of[name][::-1 if r % 2 else 1]:  # each library goes first in every other round
                call(s)  # untimed: the timed call follows one of its own kind, not the other library's or another call
                row[name][lname + "_ms"] = round(call(s)[0], 3)
        lines.append(row)
    for s in sides.values():
        s.close()
    for name in calls:
        res = out["calls"][name] = {}
        for key in lines[0][name]:
            v = [row[name][key] for row in lines]
            res[key] = {"median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
        if "parent_ms" in res:
            res["vs_parent"] = _vs_parent(res["this_ms"], res["parent_ms"])
    apart = {name: res["vs_parent"] for name, res in out["calls"].items()
             if "vs_parent" in res and not res["vs_parent"]["agree"]}
    slower = ["%s: %s" % (name, v) for name, v in apart.items() if v["median_difference_ms"] > 0]
    out["faster_than_parent"] = sorted(name for name, v in apart.items() if v["median_difference_ms"] < 0)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ab_molecules_calls_%s.jsonl" % args.tag), "w") as f:
        for row in lines:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    unequal = [name for name, same in out["outputs_equal"].items() if not same]
    assert not unequal, "outputs differ from --parent-lib: " + ", ".join(unequal)
    assert not slower, "a call is slower than --parent-lib beyond that library's own spread: " + "; ".join(slower)
    return out


def _with_umi_errors(d_umi, UL, rate, seed=17):
    """The reads' ThreeBit UMIs with every base of every read replaced by one of the three other bases
    with probability `rate` (a triplet that is no base, the N of a bad UMI, stays as it is)."""
    import torch
    g = torch.Generator(device=d_umi.device).manual_seed(seed)
    out = d_umi.clone()
    n = out.numel()
    for p in range(UL):
        t = (out >> (3 * p)) & 7
        hit = (torch.rand(n, device=out.device, generator=g) < rate) & (t >= 1) & (t <= 4)
        other = ((t - 1 + torch.randint(1, 4, (n,), device=out.device, generator=g)) & 3) + 1
        out ^= torch.where(hit, (t ^ other) << (3 * p), torch.zeros_like(t))
    return out.contiguous()


DIRECTIONAL_CALLS = UPDATE_CALLS + ("sct_molecules_collapse",)


def directional_step(args):
    """The directional clusters (collapse_device(method='directional')) on the molecules step's reads
    as drawn, with every UMI base of every read substituted with probability --umi-error, so that
    stored UMIs have neighbours.  Alternating within every round, through the C ABI, for this library
    and for the one given by --parent-lib (skipped without it): (a) the plain update, (b) the counted
    update, (c) the one-step collapse on the table (b) left; then, this library only, on the same
    table: (d) the directional call with the sweeps over the worklist (SCT_TUNE_DIRECTIONAL_FORM 1, the
    default) and (e) over the whole table (0), each with its sweeps and worklist entries.  Medians with
    min-max over --rounds; the clusters beside the one-step collapsed.  (a), (b) and (c) must not be
    slower than the parent's by more than the min-max spread of the parent's own rounds: the step
    fails, its profile written, when one is.  Every round is one line of
    profiles/ab_umi_directional.jsonl (ab_umi_directional_<tag>.jsonl for a tag other than "run"), the
    summary its last."""
    import ctypes

    import numpy as np
    import torch
    from sctools_amd import _lib

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    d_index, d_umi, _ = inputs["shuffled"]
    d_umi = _with_umi_errors(d_umi, UL, args.umi_error)
    del inputs
    torch.cuda.empty_cache()
    this, old = _lib.lib(), _parent_lib(args, DIRECTIONAL_CALLS)
    vp = ctypes.c_void_p
    d_out = torch.zeros(nw + 1, dtype=torch.int64, device=d_index.device)

    def synced(call):
        def go():
            assert call() == 0
            torch.cuda.synchronize()
        return _time_ms(go)

    def answer():
        got = d_out.cpu().tolist()
        return sum(got[:nw]), got[nw]

    def run(lib, counted, directional=False):
        """{what: ms} and {what: numbers} of one fresh counter of `lib`"""
        h = vp()
        create = lib.sct_molecules_create_counted if counted else lib.sct_molecules_create
        assert create(nw, 3, UL, hint, ctypes.byref(h)) == 0
        ms, facts = {}, {}
        try:
            ms["update"] = synced(lambda: lib.sct_molecules_update(h, vp(d_index.data_ptr()), vp(d_umi.data_ptr()), n, None))
            if counted:
                ms["collapse"] = synced(lambda: lib.sct_molecules_collapse(h, vp(d_out.data_ptr()),
                                                                           vp(d_out.data_ptr() + 8 * nw), None))
                facts["one_step"] = answer()
            for form in (1, 0) if directional else ():
                with _lib.tuning(directional_form=form):
                    ms["directional_form%d" % form] = synced(lambda: lib.sct_molecules_collapse_by(
                        h, _lib.COLLAPSE_DIRECTIONAL, vp(d_out.data_ptr()), vp(d_out.data_ptr() + 8 * nw), None))
                sweeps, listed, swept = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
                assert lib.sct_molecules_directional_info(h, ctypes.byref(sweeps), ctypes.byref(listed),
                                                          ctypes.byref(swept)) == 0
                facts["directional_form%d" % form] = answer() + (listed.value,)
                # (how far a sweep sees the labels other waves write in it is not fixed: these may differ by round)
                ms["sweeps_form%d" % form], ms["swept_form%d" % form] = sweeps.value, swept.value
            if directional:
                capacity = ctypes.c_int64()
                assert lib.sct_molecules_info(h, None, None, ctypes.byref(capacity)) == 0
                facts["capacity"] = capacity.value
            reads, molecules, tally = np.empty(nw, np.uint64), np.empty(nw, np.uint64), np.empty(3, np.uint64)
            assert lib.sct_molecules_counts_host(h, _lib._ptr(reads), _lib._ptr(molecules), _lib._ptr(tally)) == 0
            facts["counts"] = (int(reads.sum()), int(molecules.sum())) + tuple(int(t) for t in tally)
        finally:
            lib.sct_molecules_destroy(h)
        return ms, facts

    run(this, True, True)  # warm-up: code objects, pool
    if old:
        run(old, True)
    lines, facts = [], None
    for r in range(args.rounds):
        row = {"round": r, "n": n, "nw": nw, "umi_error": args.umi_error}
        for name, lib in (("this", this), ("parent", old))[::-1 if r % 2 else 1]:  # (who goes first alternates)
            if lib is None:
                continue
            plain, f_plain = run(lib, False)
            counted, f = run(lib, True, directional=lib is this)
            assert f["counts"] == f_plain["counts"], (f, f_plain)
            if lib is this:
                assert f["directional_form1"][:2] == f["directional_form0"][:2], f  # both forms: the same numbers
                row[name + "_sweeps"] = {k: v for k, v in counted.items() if k.startswith("sw")}
            known = {k: v for k, v in (facts or f).items() if k in f}
            assert f == known, (f, facts)  # every library and round: the same numbers
            facts = facts or f
            row[name] = {"plain_update_ms": round(plain["update"], 3), "counted_update_ms": round(counted["update"], 3),
                         "collapse_ms": round(counted["collapse"], 3)}
            row[name].update({k + "_ms": round(v, 3) for k, v in counted.items() if k.startswith("directional")})
        lines.append(row)
    out = {"n": n, "nw": nw, "umi_length": UL, "umi_error": args.umi_error, "capacity_hint": hint,
           "parent_lib": bool(old), "rounds": args.rounds}
    for name in ("this", "parent"):
        if name in lines[0]:
            out[name] = {}
            for key in lines[0][name]:
                a = [row[name][key] for row in lines]
                out[name][key] = {"median": round(float(np.median(a)), 3), "min": min(a), "max": max(a)}
    reads, molecules = facts["counts"][:2]
    clusters, moved, listed = facts["directional_form1"]
    out["sweeps"] = {k: {"median": float(np.median(a)), "min": min(a), "max": max(a)}
                     for k in lines[0]["this_sweeps"] for a in [[row["this_sweeps"][k] for row in lines]]}
    out.update(reads=reads, molecules=molecules, one_step_collapsed=facts["one_step"][0],
               one_step_n_corrected=facts["one_step"][1], clusters=clusters, directional_n_corrected=moved,
               worklist=listed,
               capacity=facts["capacity"], scratch_bytes=4 * facts["capacity"] + 8 * molecules + 256)
    slower = []
    if old:
        out["vs_parent"] = {k: _vs_parent(out["this"][k], out["parent"][k]) for k in out["parent"]}
        slower = ["%s: %s" % (k, v) for k, v in out["vs_parent"].items()
                  if not v["agree"] and v["median_difference_ms"] > 0]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = "ab_umi_directional.jsonl" if args.tag == "run" else "ab_umi_directional_%s.jsonl" % args.tag
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        for row in lines:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    assert not slower, "slower than --parent-lib beyond that library's own spread: " + "; ".join(slower)
    return out


DOWNSAMPLE_CALLS = UPDATE_CALLS + ("sct_molecules_collapse", "sct_molecules_merge")
DOWNSAMPLE_WAVE_READS = (64, 256, 1024, 4096)


def _skewed_counter(nw, UL, device):
    """A counted MoleculeCounter in which 0.1 % of the molecules carry half the reads: 2,000,000
    molecules of 4 reads and 2,000 of 250, 1,000, 4,000 or 16,000 (a quarter each).  (counter, reads)."""
    import torch
    from sctools_amd import counting
    light, heavy = 2_000_000, 2_000
    g = torch.Generator(device=device).manual_seed(23)
    table = torch.zeros(4096, dtype=torch.int64, device=device)  # 4096 distinct good UMI codes
    t = torch.randperm(4 ** UL, device=device, generator=g)[:4096]
    for p in range(UL):
        table |= (((t >> (2 * p)) & 3) + 1) << (3 * p)
    mol = torch.arange(light + heavy, device=device)
    per = torch.full((light + heavy,), 4, dtype=torch.int64, device=device)
    per[light:] = torch.tensor([250, 1000, 4000, 16000], device=device).repeat(heavy // 4)
    row = torch.repeat_interleave(mol, per)
    row = row[torch.randperm(row.numel(), device=device, generator=g)]
    d_index = (row % nw).to(torch.int32).contiguous()
    d_umi = table[row // nw].contiguous()
    mc = counting.MoleculeCounter(nw, UL, capacity_hint=1 << 23, read_counts=True)
    mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), row.numel())
    torch.cuda.synchronize()
    assert len(mc) == light + heavy
    return mc, int(row.numel())


def downsample_step(args):
    """Downsampling on the molecules step's reads as drawn: a counted table of all n reads, then, per
    round and on that table, downsample at fractions 0.1 and 0.5 into an empty 64-slot counter (the
    whole call, and the counting pass alone as the one-threshold curve; the insert pass is the rest),
    saturation_curve at k = 16, the one-threshold curve in the register form beside the LDS form (the
    same threshold given twice), and merge of the table into an empty counter, whose claim path is
    downsample's.  Once: the host route pairs(reads=True) + numpy binomial + update at 0.5.  Then
    SCT_TUNE_DOWNSAMPLE_WAVE_READS 64, 256, 1024 and 4096, interleaved, on a second table in which
    0.1 % of the molecules carry half the reads.  And, alternating within every round through the C
    ABI, this library and --parent-lib (skipped without it): the plain update, the counted update,
    the one-step collapse and the merge into an empty counter, which must not be slower than the
    parent's by more than the min-max spread of the parent's own rounds: the step fails, its profile
    written, when one is.  Medians with min-max over --rounds; every round is one line of
    profiles/ab_downsample.jsonl (ab_downsample_<tag>.jsonl for a tag other than "run"), the summary
    its last."""
    import ctypes

    import numpy as np
    import torch
    from sctools_amd import _lib, counting

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    d_index, d_umi, _ = inputs["shuffled"]
    del inputs
    torch.cuda.empty_cache()
    this, old = _lib.lib(), _parent_lib(args, DOWNSAMPLE_CALLS)
    vp = ctypes.c_void_p
    d_out = torch.zeros(nw + 1, dtype=torch.int64, device=d_index.device)
    d_curve = torch.zeros(2 * 64, dtype=torch.int64, device=d_index.device)

    def synced(call):
        def go():
            assert call() in (0, None)
            torch.cuda.synchronize()
        return _time_ms(go)

    def run(lib, counted):
        """{what: ms} and the counts of one fresh counter of `lib`, through the C ABI"""
        h, e = vp(), vp()
        create = lib.sct_molecules_create_counted if counted else lib.sct_molecules_create
        assert create(nw, 3, UL, hint, ctypes.byref(h)) == 0
        assert create(nw, 3, UL, 64, ctypes.byref(e)) == 0
        ms = {}
        try:
            ms["update"] = synced(lambda: lib.sct_molecules_update(h, vp(d_index.data_ptr()), vp(d_umi.data_ptr()), n, None))
            if counted:
                ms["collapse"] = synced(lambda: lib.sct_molecules_collapse(h, vp(d_out.data_ptr()),
                                                                           vp(d_out.data_ptr() + 8 * nw), None))
                ms["merge"] = synced(lambda: lib.sct_molecules_merge(e, h, None))
            reads, molecules, tally = np.empty(nw, np.uint64), np.empty(nw, np.uint64), np.empty(3, np.uint64)
            assert lib.sct_molecules_counts_host(h, _lib._ptr(reads), _lib._ptr(molecules), _lib._ptr(tally)) == 0
        finally:
            lib.sct_molecules_destroy(h)
            lib.sct_molecules_destroy(e)
        return ms, (int(reads.sum()), int(molecules.sum())) + tuple(int(t) for t in tally)

    def curve_ms(mc, thresholds):
        return synced(lambda: mc.saturation_curve_device(thresholds, d_curve.data_ptr(), d_curve.data_ptr() + 8 * 64))

    def thin_ms(mc, threshold):
        """(ms, (molecules, total, capacity)) of downsample into an empty 64-slot counter"""
        with counting.MoleculeCounter(nw, UL, capacity_hint=64, read_counts=True) as into:
            ms = synced(lambda: (mc.downsample_device(into, threshold), None)[1])
            info = into.info()
        return ms, (info["nmolecules"], info["total"], info["capacity"])

    table = counting.MoleculeCounter(nw, UL, capacity_hint=hint, read_counts=True)
    table.update_device(d_index.data_ptr(), d_umi.data_ptr(), n)
    torch.cuda.synchronize()
    fractions = {"0.1": counting.downsample_threshold(0.1), "0.5": counting.downsample_threshold(0.5)}
    points = [counting.downsample_threshold((t + 1) / 16) for t in range(16)]
    skewed, skewed_reads = _skewed_counter(nw, UL, d_index.device)

    def this_only():
        ms, facts = {}, {}
        for name, threshold in fractions.items():
            ms["downsample_%s" % name], facts["downsample_%s" % name] = thin_ms(table, threshold)
            ms["count_pass_%s" % name] = curve_ms(table, [threshold])
            ms["insert_pass_%s" % name] = ms["downsample_%s" % name] - ms["count_pass_%s" % name]
            facts["curve_%s" % name] = (int(d_curve[0]), int(d_curve[64]))
            ms["count_pass_lds_form_%s" % name] = curve_ms(table, [threshold, threshold])
            assert facts["curve_%s" % name] == (int(d_curve[0]), int(d_curve[64])) == (int(d_curve[1]), int(d_curve[65]))
        ms["curve_k16"] = curve_ms(table, points)
        facts["curve_k16"] = (d_curve[:16].tolist(), d_curve[64:80].tolist())
        for w in DOWNSAMPLE_WAVE_READS:
            with _lib.tuning(downsample_wave_reads=w):
                ms["skewed_downsample_0.5_w%d" % w], f = thin_ms(skewed, fractions["0.5"])
                ms["skewed_curve_k16_w%d" % w] = curve_ms(skewed, points)
            f = (f, d_curve[:16].tolist(), d_curve[64:80].tolist())
            assert facts.setdefault("skewed", f) == f, (w, f)  # every W: the same numbers
        return ms, facts

    def host_route(threshold):
        """the rows fetched, thinned by numpy and replayed through update: {part: ms}"""
        out = {}
        t = time.perf_counter()
        index, umi, reads = table.pairs(reads=True)
        out["pairs_ms"] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        kept = np.random.default_rng(0).binomial(reads, threshold / 2 ** 32)
        index, umi = np.repeat(index, kept), np.repeat(umi, kept)
        out["numpy_ms"] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        with counting.MoleculeCounter(nw, UL, capacity_hint=64, read_counts=True) as into:
            into.update(index, umi)
            out["molecules"] = len(into)
        out["update_ms"] = (time.perf_counter() - t) * 1e3
        out["total_ms"] = out["pairs_ms"] + out["numpy_ms"] + out["update_ms"]
        return {k: round(v, 3) for k, v in out.items()}

    run(this, True)  # warm-up: code objects, pool
    this_only()
    if old:
        run(old, True)
    lines, facts, counts = [], None, None
    for r in range(args.rounds):
        row = {"round": r, "n": n, "nw": nw}
        for name, lib in (("this", this), ("parent", old))[::-1 if r % 2 else 1]:  # (who goes first alternates)
            if lib is None:
                continue
            plain, c_plain = run(lib, False)
            counted, c = run(lib, True)
            assert c == c_plain == (counts or c), (c, c_plain, counts)  # every library and round: the same numbers
            counts = c
            row[name] = {"plain_update_ms": round(plain["update"], 3), "counted_update_ms": round(counted["update"], 3),
                         "collapse_ms": round(counted["collapse"], 3), "merge_ms": round(counted["merge"], 3)}
        ms, f = this_only()
        assert f == (facts or f), (f, facts)
        facts = f
        row["downsample"] = {k + "_ms": round(v, 3) for k, v in ms.items()}
        lines.append(row)
    host = host_route(fractions["0.5"])
    out = {"n": n, "nw": nw, "umi_length": UL, "capacity_hint": hint, "parent_lib": bool(old), "rounds": args.rounds,
           "reads": counts[0], "molecules": counts[1], "table_capacity": table.info()["capacity"],
           "skewed": {"reads": skewed_reads, "molecules": len(skewed), "capacity": skewed.info()["capacity"]},
           "host_route_0.5": host}
    table.close()
    skewed.close()
    for name in ("this", "parent", "downsample"):
        if name in lines[0]:
            out[name] = {}
            for key in lines[0][name]:
                a = [row[name][key] for row in lines]
                out[name][key] = {"median": round(float(np.median(a)), 3), "min": min(a), "max": max(a)}
    for name in fractions:
        molecules, total, capacity = facts["downsample_%s" % name]
        out["kept_%s" % name] = {"molecules": molecules, "total": total, "capacity": capacity,
                                 "curve": facts["curve_%s" % name]}
    out["curve_k16"] = {"reads": facts["curve_k16"][0], "molecules": facts["curve_k16"][1]}
    sweep = {w: out["downsample"]["skewed_downsample_0.5_w%d_ms" % w]["median"]
             + out["downsample"]["skewed_curve_k16_w%d_ms" % w]["median"] for w in DOWNSAMPLE_WAVE_READS}
    out["wave_reads_sweep_ms"] = {str(w): round(v, 3) for w, v in sweep.items()}
    out["wave_reads_best"] = min(sweep, key=sweep.get)
    slower = []
    if old:
        out["vs_parent"] = {k: _vs_parent(out["this"][k], out["parent"][k]) for k in out["parent"]}
        slower = ["%s: %s" % (k, v) for k, v in out["vs_parent"].items()
                  if not v["agree"] and v["median_difference_ms"] > 0]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = "ab_downsample.jsonl" if args.tag == "run" else "ab_downsample_%s.jsonl" % args.tag
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        for row in lines:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    assert not slower, "slower than --parent-lib beyond that library's own spread: " + "; ".join(slower)
    return out


RESOLVE_PARENT_CALLS = ("sct_tune_set", "sct_molecules_create_features", "sct_molecules_update_features",
                        "sct_molecules_info", "sct_molecules_matrix", "sct_molecules_destroy")


def _resolve_on_host(rows, nw, nf):
    """The host route of resolving features: (resolved[nw], (n_shared, n_lost, n_tied, reads_dropped),
    kept cells index * nf + feature ascending, kept molecules per such cell) from the rows
    (index, feature, image umi, reads) by np.lexsort and reduceat."""
    import numpy as np
    index, feature, image, reads = rows
    order = np.lexsort((feature, image, index))
    index, feature, image, reads = index[order], feature[order], image[order], reads[order]
    group_change = np.empty(index.size, bool)
    group_change[0] = True
    group_change[1:] = (index[1:] != index[:-1]) | (image[1:] != image[:-1])
    molecule_head = group_change.copy()
    molecule_head[1:] |= feature[1:] != feature[:-1]
    starts = np.flatnonzero(molecule_head)
    m_reads = np.add.reduceat(reads, starts)  # the collapsed molecules, in (index, image, feature) order
    m_index, m_feature = index[starts], feature[starts]
    group_starts = np.flatnonzero(group_change[starts])
    members = np.diff(np.append(group_starts, starts.size))
    top = np.maximum.reduceat(m_reads, group_starts)
    at_top = m_reads == np.repeat(top, members)
    unique = np.add.reduceat(at_top.astype(np.int64), group_starts) == 1
    kept = at_top & np.repeat(unique, members)
    resolved = np.bincount(m_index[kept], minlength=nw).astype(np.int64)
    tally = (int((members >= 2).sum()), int((members[unique] - 1).sum()), int(members[~unique].sum()),
             int(m_reads.sum() - top[unique].sum()))
    cells, per_cell = np.unique(m_index[kept].astype(np.int64) * nf + m_feature[kept], return_counts=True)
    return resolved, tally, cells, per_cell


def resolve_step(args):
    """Resolving features on the matrix step's reads (nf = 4096, every feature in use) with a share
    --hop of the reads moved to another feature drawn uniformly: without hops a molecule's feature is a
    function of its (barcode, UMI) and nothing is shared.  On the table the counted feature update
    left, alternating within every round: resolve_device for the three methods, matrix_device with
    every column and the resolved one (one_step and directional; molecules, reads and resolved for
    none), matrix_device with molecules, reads and collapsed as it was, and the host route on the same
    counter -- pairs(features=True, reads=True, parents=True) and np.lexsort + reduceat (one_step every
    round, the yardstick; none and directional once).  Device and host answers must be equal.  With
    --parent-lib, sct_molecules_matrix with every column runs first, alternating in both libraries
    (the order swapped every round), each on its own counter of the same reads: the medians agree when they differ by no more than the min-max
    spread of the parent's own rounds, and the outputs are equal element for element; the step fails
    (its profile written) when they are not.  Every round is one line of the profile, the summary its
    last (profiles/ab_feature_resolve.jsonl, or ab_feature_resolve_<tag>.jsonl)."""
    import ctypes

    import numpy as np
    import torch
    from sctools_amd import _lib, counting

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    nf = 4096
    dev = torch.device("cuda")
    old = _parent_lib(args, RESOLVE_PARENT_CALLS)
    di, du, _ = inputs["shuffled"]
    df = _features_of(di, du, nf, nf)
    g = torch.Generator(device=dev).manual_seed(29)
    hops = (torch.rand(n, device=dev, generator=g) < args.hop) & (df >= 0)
    other = (df + 1 + torch.randint(0, nf - 1, (n,), device=dev, generator=g, dtype=torch.int32)) % nf
    df = torch.where(hops, other, df).contiguous()
    n_hopped = int(hops.sum())
    del hops, other
    mc = counting.MoleculeCounter(nw, UL, capacity_hint=hint, read_counts=True, features=nf)
    mc.update_device(di.data_ptr(), du.data_ptr(), n, feature_ptr=df.data_ptr())
    nmol = len(mc)
    methods = ("none", "one_step", "directional")
    d_resolved = torch.empty((3, nw), dtype=torch.int64, device=dev)
    d_tally = torch.empty((3, 4), dtype=torch.int64, device=dev)
    o_indptr = torch.empty(nw + 1, dtype=torch.int64, device=dev)
    o_feat = torch.empty(nmol, dtype=torch.int32, device=dev)
    o_val = torch.empty((4, nmol), dtype=torch.int64, device=dev)
    got = {}

    def run_resolve(k):
        def go():
            mc.resolve_device(d_resolved[k].data_ptr(), d_tally[k].data_ptr(), method=methods[k])
            torch.cuda.synchronize()
        return _time_ms(go)

    def run_matrix(method, resolved):
        collapsed = o_val[2].data_ptr() if method != "none" else None
        def go():
            got["nnz"] = mc.matrix_device(o_indptr.data_ptr(), o_feat.data_ptr(), o_val[0].data_ptr(),
                                          o_val[1].data_ptr(), collapsed, nmol, method=method,
                                          resolved_ptr=o_val[3].data_ptr() if resolved else None)
            torch.cuda.synchronize()
        return _time_ms(go)

    def host_route(method):
        """(pairs ms, numpy ms, the host answer)"""
        rows = {}
        if method == "none":
            pairs_ms = _time_ms(lambda: rows.update(r=mc.pairs(features=True, reads=True)))
            pi, pf, pu, pr = rows["r"]
            image = pu
        else:
            pairs_ms = _time_ms(lambda: rows.update(r=mc.pairs(features=True, reads=True, parents=True, method=method)))
            pi, pf, _, pr, image = rows["r"]
        numpy_ms = _time_ms(lambda: rows.update(a=_resolve_on_host((pi, pf, image, pr), nw, nf)))
        return pairs_ms, numpy_ms, rows["a"]

    # the untouched matrix call beside the parent library's, each on a counter of its own library
    vp = ctypes.c_void_p
    handles = {}
    if old:
        p_indptr, p_feat, p_val = torch.empty_like(o_indptr), torch.empty_like(o_feat), torch.empty_like(o_val[:3])
        for lname, lib in (("this", _lib.lib()), ("parent", old)):
            h = vp()
            assert lib.sct_molecules_create_features(nw, nf, 3, UL, hint, 1, -1, ctypes.byref(h)) == 0
            assert lib.sct_molecules_update_features(h, vp(di.data_ptr()), vp(df.data_ptr()), vp(du.data_ptr()), n, None) == 0
            handles[lname] = (lib, h)

    def run_abi_matrix(lname, out_indptr, out_feat, out_val):
        lib, h = handles[lname]
        nnz = ctypes.c_int64(0)
        def go():
            assert lib.sct_molecules_matrix(h, vp(out_indptr.data_ptr()), vp(out_feat.data_ptr()), vp(out_val[0].data_ptr()),
                                            vp(out_val[1].data_ptr()), vp(out_val[2].data_ptr()), nmol, ctypes.byref(nnz),
                                            None) == 0
            torch.cuda.synchronize()
        ms = _time_ms(go)
        return ms, nnz.value

    # (first, before this library's pool has served a resolve call the parent's never sees, and in
    # alternating order: whichever library runs second in a round runs first in the next)
    abi_rounds = []
    if old:
        abi = {"this": lambda: run_abi_matrix("this", o_indptr, o_feat, o_val)[0],
               "parent": lambda: run_abi_matrix("parent", p_indptr, p_feat, p_val)[0]}
        abi["this"](), abi["parent"]()  # warm-up
        for r in range(args.rounds):
            order = ("this", "parent") if r % 2 == 0 else ("parent", "this")
            abi_rounds.append({"abi_matrix_%s_ms" % lname: round(abi[lname](), 3) for lname in order})
    for k in range(3):
        run_resolve(k)  # warm-up
    run_matrix("one_step", True), run_matrix("one_step", False)
    rounds, host = [], {}
    for r in range(args.rounds):
        row = {"what": "resolve", "round": r}
        for k, method in enumerate(methods):
            row["resolve_%s_ms" % method] = round(run_resolve(k), 3)
        for method in methods:
            row["matrix_resolved_%s_ms" % method] = round(run_matrix(method, True), 3)
        row["matrix_reads_collapsed_ms"] = round(run_matrix("one_step", False), 3)
        if old:
            row.update(abi_rounds[r])
        pairs_ms, numpy_ms, host["one_step"] = host_route("one_step")
        row["host_pairs_ms"], row["host_lexsort_reduceat_ms"] = round(pairs_ms, 1), round(numpy_ms, 1)
        row["host_route_ms"] = round(pairs_ms + numpy_ms, 1)
        rounds.append(row)
    out = {"n": n, "nw": nw, "nf": nf, "umi_length": UL, "capacity_hint": hint, "hop": args.hop, "hopped_reads": n_hopped,
           "molecules": nmol, "capacity": mc.info()["capacity"], "rounds": args.rounds, "parent_lib": bool(old)}
    for key in rounds[0]:
        if key.endswith("_ms"):
            v = [row[key] for row in rounds]
            out[key] = {"median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
    out["host_route_once_ms"] = {}
    for method in ("none", "directional"):
        pairs_ms, numpy_ms, host[method] = host_route(method)
        out["host_route_once_ms"][method] = round(pairs_ms + numpy_ms, 1)
    # device == host, for every method: resolve(), and the matrix's resolved column
    equal = {}
    for k, method in enumerate(methods):
        h_resolved, h_tally, h_cells, h_per_cell = host[method]
        run_resolve(k)
        run_matrix(method, True)
        nnz = got["nnz"]
        rows_of = torch.repeat_interleave(torch.arange(nw, device=dev), o_indptr[1:] - o_indptr[:-1])
        kept = o_val[3, :nnz]
        cells = (rows_of * nf + o_feat[:nnz])[kept > 0].cpu().numpy()
        equal[method] = bool(np.array_equal(d_resolved[k].cpu().numpy(), h_resolved)
                             and tuple(d_tally[k].cpu().tolist()) == h_tally and np.array_equal(cells, h_cells)
                             and np.array_equal(kept[kept > 0].cpu().numpy(), h_per_cell)
                             and int(kept.sum()) == int(h_resolved.sum()))
        out["answer_" + method] = {"resolved": int(h_resolved.sum()), "n_shared": h_tally[0], "n_lost": h_tally[1],
                                   "n_tied": h_tally[2], "reads_dropped": h_tally[3], "nnz": nnz,
                                   "explicit_zeros": int((kept == 0).sum())}
    out["device_equals_host"] = equal
    out["host_route_over_resolve"] = round(out["host_route_ms"]["median"] / out["resolve_one_step_ms"]["median"], 1)
    out["host_route_over_matrix_resolved"] = round(out["host_route_ms"]["median"]
                                                   / out["matrix_resolved_one_step_ms"]["median"], 1)
    out["matrix_resolved_over_matrix"] = round(out["matrix_resolved_one_step_ms"]["median"]
                                               / out["matrix_reads_collapsed_ms"]["median"], 2)
    if old:
        n_this, n_parent = run_abi_matrix("this", o_indptr, o_feat, o_val)[1], run_abi_matrix("parent", p_indptr, p_feat, p_val)[1]
        out["abi_matrix_outputs_equal"] = bool(n_this == n_parent and torch.equal(o_indptr, p_indptr)
                                               and torch.equal(o_feat[:n_this], p_feat[:n_this])
                                               and torch.equal(o_val[:3, :n_this], p_val[:, :n_this]))
        out["abi_matrix_vs_parent"] = _vs_parent(out["abi_matrix_this_ms"], out["abi_matrix_parent_ms"])
        for lib, h in handles.values():
            lib.sct_molecules_destroy(h)
    mc.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = "ab_feature_resolve.jsonl" if args.tag == "run" else "ab_feature_resolve_%s.jsonl" % args.tag
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        for row in rounds:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    assert all(equal.values()), "the device and the host route disagree: %r" % (equal,)
    if old:
        assert out["abi_matrix_outputs_equal"], "sct_molecules_matrix differs from --parent-lib"
        assert out["abi_matrix_vs_parent"]["agree"], ("sct_molecules_matrix differs from --parent-lib beyond that "
                                                      "library's own spread: %r" % (out["abi_matrix_vs_parent"],))
    return out


GROUPS_PARENT_CALLS = ("sct_tune_set", "sct_molecules_create", "sct_molecules_create_counted", "sct_molecules_update",
                       "sct_molecules_create_features", "sct_molecules_update_features", "sct_molecules_info",
                       "sct_molecules_collapse", "sct_molecules_resolve", "sct_molecules_matrix",
                       "sct_molecules_destroy")


def _groups_on_host(rows, reads, nf, umi_bits, resolved):
    """The host route of tagging reads: (final_umi uint64, status uint8, mol_reads int64, first bool) of
    the reads (index, feature, umi) from the counter's rows (index, feature, umi, reads, image umi) in
    key order -- key packing and np.searchsorted for the stored key, np.unique + bincount for the final
    molecules' reads, the winner rule by np.lexsort and reduceat, np.unique(return_index=True) for first."""
    import numpy as np
    pi, pf, pu, pr, image = rows
    ri, rf, ru = reads
    umi_mask = np.int64((1 << umi_bits) - 1)
    keys = ((pi.astype(np.int64) * nf + pf) << umi_bits) | pu.view(np.int64)
    # the final molecules: the rows' keys under their images
    final_keys, row_mol = np.unique((keys & ~umi_mask) | image.view(np.int64), return_inverse=True)
    mol_reads = np.bincount(row_mol, weights=pr.astype(np.float64), minlength=final_keys.size).astype(np.int64)
    kept = np.ones(final_keys.size, bool)
    if resolved:
        m_feature = (final_keys >> umi_bits) & (nf - 1)
        group = ((final_keys >> umi_bits) // nf << umi_bits) | (final_keys & umi_mask)  # (index, image)
        order = np.lexsort((m_feature, group))
        g_sorted, r_sorted = group[order], mol_reads[order]
        head = np.empty(order.size, bool)
        head[0] = True
        head[1:] = g_sorted[1:] != g_sorted[:-1]
        starts = np.flatnonzero(head)
        members = np.diff(np.append(starts, order.size))
        top = np.maximum.reduceat(r_sorted, starts)
        at_top = r_sorted == np.repeat(top, members)
        unique = np.add.reduceat(at_top.astype(np.int64), starts) == 1
        kept[order] = at_top & np.repeat(unique, members)
    # the reads
    status = np.zeros(ri.size, np.uint8)
    ones = np.uint64(0x1249249249249249 & ((1 << umi_bits) - 1))
    bad_umi = ((ru >> np.uint64(umi_bits)) != 0) | ((((ru >> np.uint64(2)) ^ ((ru >> np.uint64(1)) | ru)) & ones) != ones)
    good = (ri >= 0) & ~bad_umi & (rf >= 0)
    status[rf < 0] = 4
    status[bad_umi] = 3
    status[ri == -2] = 2
    status[ri == -1] = 1
    at = np.flatnonzero(good)
    rkey = ((ri[at].astype(np.int64) * nf + rf[at]) << umi_bits) | ru[at].view(np.int64)
    pos = np.minimum(np.searchsorted(keys, rkey), keys.size - 1)
    found = keys[pos] == rkey
    status[at[~found]] = 5
    at, mol = at[found], row_mol[pos[found]]
    status[at[~kept[mol]]] = 6
    final = ru.copy()
    final[at] = (final_keys[mol] & umi_mask).view(np.uint64)
    out_reads = np.zeros(ri.size, np.int64)
    out_reads[at] = mol_reads[mol]
    first = np.zeros(ri.size, bool)
    grouped = kept[mol]
    _, where = np.unique(mol[grouped], return_index=True)
    first[at[grouped][where]] = True
    return final, status, out_reads, first


def groups_step(args):
    """Read groups on the resolve step's input (nf = 4096, --hop of the reads moved to another feature),
    against the table the counted feature update left.  Alternating within every round: read_groups()
    for the three methods with and without resolved (every column); tag_device of all the reads in one
    batch, as the other steps feed them, with no optional column, with reads, and with reads and first
    (one_step, resolved); update_features of the same reads into a fresh counter -- the same access
    pattern plus atomics; and with --parent-lib the plain, counted and feature updates, the collapse,
    resolve and the matrix through the C ABI in this library and in that one, the order swapped every
    round (they agree when the medians differ by no more than the min-max spread of the parent's own
    rounds; a call that does not is named in the summary).  Once, the host route -- pairs(features=True,
    reads=True, parents=True), key packing and np.searchsorted, np.lexsort + reduceat, np.unique -- whose
    four columns must equal the device's.  Every round is one line of the profile, the summary its
    last (profiles/ab_read_groups.jsonl, or ab_read_groups_<tag>.jsonl)."""
    import ctypes

    import numpy as np
    import torch
    from sctools_amd import _lib, counting

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    nf = 4096
    dev = torch.device("cuda")
    this, old = _lib.lib(), _parent_lib(args, GROUPS_PARENT_CALLS)
    di, du, _ = inputs["shuffled"]
    df = _features_of(di, du, nf, nf)
    g = torch.Generator(device=dev).manual_seed(29)
    hops = (torch.rand(n, device=dev, generator=g) < args.hop) & (df >= 0)
    other = (df + 1 + torch.randint(0, nf - 1, (n,), device=dev, generator=g, dtype=torch.int32)) % nf
    df = torch.where(hops, other, df).contiguous()
    del hops, other, inputs
    mc = counting.MoleculeCounter(nw, UL, capacity_hint=hint, read_counts=True, features=nf)
    mc.update_device(di.data_ptr(), du.data_ptr(), n, feature_ptr=df.data_ptr())
    nmol = len(mc)
    methods = ("none", "one_step", "directional")
    o_final = torch.empty(n, dtype=torch.int64, device=dev)
    o_reads = torch.empty(n, dtype=torch.int64, device=dev)
    o_status = torch.empty(n, dtype=torch.uint8, device=dev)
    o_first = torch.empty(n, dtype=torch.uint8, device=dev)
    name = "ab_read_groups.jsonl" if args.tag == "run" else "ab_read_groups_%s.jsonl" % args.tag
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    profile = open(os.path.join(ROOT, "profiles", name), "w")

    def run_create(method, resolved):
        made = {}
        def go():
            made["g"] = mc.read_groups(method=method, resolved=resolved, reads=True, first=True)
            torch.cuda.synchronize()
        ms = _time_ms(go)
        made["g"].close()
        return ms

    forms = {"plain": dict(), "reads": dict(reads=True), "reads_first": dict(reads=True, first=True)}
    taggers = {k: mc.read_groups(method="one_step", resolved=True, **kw) for k, kw in forms.items()}

    def run_tag(groups):
        def go():
            groups.tag_device(di.data_ptr(), du.data_ptr(), n, o_final.data_ptr(), o_status.data_ptr(),
                              reads_ptr=o_reads.data_ptr() if groups.reads else None,
                              first_ptr=o_first.data_ptr() if groups.first else None, feature_ptr=df.data_ptr())
            torch.cuda.synchronize()
        return _time_ms(go)

    vp = ctypes.c_void_p

    def run_update(lib, what):
        """ms of one update of all the reads into a fresh counter of `lib`: plain, counted or features (counted)"""
        h = vp()
        if what == "features":
            assert lib.sct_molecules_create_features(nw, nf, 3, UL, hint, 1, -1, ctypes.byref(h)) == 0
        else:
            create = lib.sct_molecules_create_counted if what == "counted" else lib.sct_molecules_create
            assert create(nw, 3, UL, hint, ctypes.byref(h)) == 0
        try:
            def go():
                if what == "features":
                    assert lib.sct_molecules_update_features(h, vp(di.data_ptr()), vp(df.data_ptr()), vp(du.data_ptr()), n,
                                                             None) == 0
                else:
                    assert lib.sct_molecules_update(h, vp(di.data_ptr()), vp(du.data_ptr()), n, None) == 0
                torch.cuda.synchronize()
            return _time_ms(go)
        finally:
            lib.sct_molecules_destroy(h)

    # the read-back calls of both libraries, each on a feature counter of its own library
    libs = {"this": this}
    if old:
        libs["parent"] = old
    handles, outs = {}, {}
    for lname, lib in libs.items():
        h = vp()
        assert lib.sct_molecules_create_features(nw, nf, 3, UL, hint, 1, -1, ctypes.byref(h)) == 0
        assert lib.sct_molecules_update_features(h, vp(di.data_ptr()), vp(df.data_ptr()), vp(du.data_ptr()), n, None) == 0
        handles[lname] = h
        outs[lname] = {"collapsed": torch.empty(nw, dtype=torch.int64, device=dev),
                       "resolved": torch.empty(nw, dtype=torch.int64, device=dev),
                       "tally": torch.empty(4, dtype=torch.int64, device=dev),
                       "indptr": torch.empty(nw + 1, dtype=torch.int64, device=dev),
                       "feature": torch.empty(nmol, dtype=torch.int32, device=dev),
                       "values": torch.empty((3, nmol), dtype=torch.int64, device=dev)}

    def run_call(lname, what):
        lib, h, o = libs[lname], handles[lname], outs[lname]
        nnz = ctypes.c_int64(0)
        def go():
            if what == "collapse":
                rc = lib.sct_molecules_collapse(h, vp(o["collapsed"].data_ptr()), None, None)
            elif what == "resolve":
                rc = lib.sct_molecules_resolve(h, _lib.COLLAPSE_ONE_STEP, vp(o["resolved"].data_ptr()),
                                               vp(o["tally"].data_ptr()), None)
            else:
                v = o["values"]
                rc = lib.sct_molecules_matrix(h, vp(o["indptr"].data_ptr()), vp(o["feature"].data_ptr()),
                                              vp(v[0].data_ptr()), vp(v[1].data_ptr()), vp(v[2].data_ptr()), nmol,
                                              ctypes.byref(nnz), None)
            assert rc == 0
            torch.cuda.synchronize()
        return _time_ms(go)

    existing = [("update_%s" % w, lambda lname, w=w: run_update(libs[lname], w)) for w in ("plain", "counted", "features")]
    existing += [(w, lambda lname, w=w: run_call(lname, w)) for w in ("collapse", "resolve", "matrix")]
    # warm-up: every call once
    for k in taggers:
        run_tag(taggers[k])
    run_create("one_step", True)
    for lname in libs:
        for _, call in existing:
            call(lname)
    rounds = []
    for r in range(args.rounds):
        row = {"what": "groups", "round": r}
        for method in methods:
            for resolved in (False, True):
                row["create_%s%s_ms" % (method, "_resolved" if resolved else "")] = round(run_create(method, resolved), 3)
        for k in taggers:
            row["tag_%s_ms" % k] = round(run_tag(taggers[k]), 3)
        order = list(libs) if r % 2 == 0 else list(libs)[::-1]
        for what, call in existing:
            for lname in order:
                row["%s_%s_ms" % (what, lname)] = round(call(lname), 3)
        rounds.append(row)
        profile.write(json.dumps(row, sort_keys=True) + "\n")
        profile.flush()
    for groups in taggers.values():
        groups.close()
    out = {"n": n, "nw": nw, "nf": nf, "umi_length": UL, "capacity_hint": hint, "hop": args.hop, "molecules": nmol,
           "capacity": mc.info()["capacity"], "rounds": args.rounds, "parent_lib": bool(old)}
    for key in rounds[0]:
        if key.endswith("_ms"):
            v = [row[key] for row in rounds]
            out[key] = {"median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
    out["tag_plain_over_update_features"] = round(out["tag_plain_ms"]["median"] / out["update_features_this_ms"]["median"], 3)
    if old:
        out["vs_parent"] = {what: _vs_parent(out["%s_this_ms" % what], out["%s_parent_ms" % what]) for what, _ in existing}
        out["apart_from_parent"] = sorted(what for what, v in out["vs_parent"].items() if not v["agree"])
        o, p = outs["this"], outs["parent"]
        out["abi_outputs_equal"] = bool(torch.equal(o["collapsed"], p["collapsed"]) and torch.equal(o["resolved"], p["resolved"])
                                        and torch.equal(o["tally"], p["tally"]) and torch.equal(o["indptr"], p["indptr"]))
    for lname, lib in libs.items():
        lib.sct_molecules_destroy(handles[lname])
    del outs
    # the host route, once (one_step, resolved, every column), and its answers beside the device's
    with mc.read_groups(method="one_step", resolved=True, reads=True, first=True) as groups:
        run_tag(groups)
        tally = groups.tally().tolist()
    host = {}
    host["pairs_ms"] = round(_time_ms(lambda: host.update(rows=mc.pairs(features=True, reads=True, parents=True))), 1)
    host["reads_to_host_ms"] = round(_time_ms(lambda: host.update(
        reads=(di.cpu().numpy(), df.cpu().numpy(), du.cpu().numpy().view(np.uint64)))), 1)
    host["numpy_ms"] = round(_time_ms(lambda: host.update(a=_groups_on_host(host["rows"], host["reads"], nf, 3 * UL, True))), 1)
    h_final, h_status, h_reads, h_first = host.pop("a")
    del host["rows"], host["reads"]
    host["total_ms"] = round(host["pairs_ms"] + host["reads_to_host_ms"] + host["numpy_ms"], 1)
    out["host_route_once"] = host
    out["groups_device_equals_host"] = {
        "final_umi": bool(np.array_equal(o_final.cpu().numpy().view(np.uint64), h_final)),
        "status": bool(np.array_equal(o_status.cpu().numpy(), h_status)),
        "mol_reads": bool(np.array_equal(o_reads.cpu().numpy(), h_reads)),
        "first": bool(np.array_equal(o_first.cpu().numpy().astype(bool), h_first))}
    out["tally"] = tally
    out["moved_reads"] = int((h_final != du.cpu().numpy().view(np.uint64)).sum())
    out["first_reads"] = int(h_first.sum())
    out["host_route_over_tag_reads_first"] = round(host["total_ms"] / out["tag_reads_first_ms"]["median"], 1)
    mc.close()
    profile.write(json.dumps(out, sort_keys=True) + "\n")
    profile.close()
    assert all(out["groups_device_equals_host"].values()), "the device and the host route disagree: %r" % (
        out["groups_device_equals_host"],)
    if old:
        assert out["abi_outputs_equal"], "an existing call's outputs differ from --parent-lib"
    return out


SWAPPED_PARENT_CALLS = GROUPS_PARENT_CALLS + ("sct_molecules_merge", "sct_molecules_downsample",
                                               "sct_read_groups_create", "sct_read_groups_tag", "sct_read_groups_destroy")


def _swapped_on_host(tables, num, den):
    """The host route of removing swapped molecules: per sample (kept keys ascending, their reads,
    [shared, removed, removed reads]) from every sample's (packed keys ascending, reads) -- np.unique over
    all keys, np.searchsorted per sample, the judgement in Python integers where a product could pass
    2^63 and in int64 otherwise."""
    import numpy as np
    keys = np.unique(np.concatenate([k for k, _ in tables]))
    per = np.zeros((len(tables), keys.size), np.int64)
    for t, (k, r) in enumerate(tables):
        per[t, np.searchsorted(keys, k)] = r
    total = per.sum(axis=0)
    assert int(total.max()) * max(num, den) < 2 ** 63
    out = []
    for t, (k, r) in enumerate(tables):
        others = (total - per[t])[np.searchsorted(keys, k)]
        keep = r * (den - num) >= num * others
        out.append((k[keep], r[keep], [int((others > 0).sum()), int((~keep).sum()), int(r[~keep].sum())]))
    return out


def swapped_step(args):
    """Removing swapped molecules on the molecules step's reads as drawn, split over s = 2 and s = 4
    counted counters: a molecule's reads go to the sample its key hashes to, and --hop of the reads to
    another sample, drawn uniformly.  Per round and s: remove_swapped_device of every sample into an
    empty 64-slot counter (the device time per sample, and their sum, the whole call), and the merge of
    the same s counters into one empty counter as a yardstick, with the ratio to it; there is no pass
    mark.  Once per s, the host route -- pairs(reads=True) of every counter, key packing, np.unique and
    np.searchsorted -- whose kept molecules, reads and tallies must equal the device's.  With
    --parent-lib, alternating within every round through the C ABI in this library and in that one: the
    plain, counted and feature updates, the collapse, merge, downsample at 0.5, matrix, resolve, and
    read groups (create and tag); they agree when the medians differ by no more than the min-max spread
    of the parent's own rounds, and a call that does not is named in the summary.  Every round is one
    line of the profile, the summary its last (profiles/ab_swapped.jsonl, or ab_swapped_<tag>.jsonl)."""
    import ctypes

    import numpy as np
    import torch
    from sctools_amd import _lib, counting

    nw, UL, n, hint, pool, inputs = _molecules_input(args)
    dev = torch.device("cuda")
    this, old = _lib.lib(), _parent_lib(args, SWAPPED_PARENT_CALLS)
    di, du, dk = inputs["shuffled"]
    del inputs
    num, den = 4, 5
    g = torch.Generator(device=dev).manual_seed(31)
    mixed = (dk * -7046029254386353131) >> 33  # a molecule's hash: its home sample is this modulo s
    hops = torch.rand(n, device=dev, generator=g) < args.hop
    jump = torch.randint(1, 4, (n,), device=dev, generator=g)
    name = "ab_swapped.jsonl" if args.tag == "run" else "ab_swapped_%s.jsonl" % args.tag
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    profile = open(os.path.join(ROOT, "profiles", name), "w")

    def synced(call):
        def go():
            call()
            torch.cuda.synchronize()
        return _time_ms(go)

    samples = {}
    for s in (2, 4):
        side = torch.where(hops, (mixed + 1 + jump % (s - 1)) % s, mixed % s)
        made = []
        for t in range(s):
            at = side == t
            ti, tu = di[at].contiguous(), du[at].contiguous()
            mc = counting.MoleculeCounter(nw, UL, capacity_hint=max(64, hint // s), read_counts=True)
            mc.update_device(ti.data_ptr(), tu.data_ptr(), ti.numel())
            torch.cuda.synchronize()
            made.append(mc)
            del ti, tu, at
        samples[s] = made
        del side
    del hops, jump, mixed, dk
    torch.cuda.empty_cache()

    def run_swapped(s, keep=False):
        """({what: ms}, tallies[, the cleaned counters]) of one removal over the s samples"""
        ms, tallies, cleaned = {}, [], []
        for k, mc in enumerate(samples[s]):
            into = counting.MoleculeCounter(nw, UL, capacity_hint=64, read_counts=True)
            others = samples[s][:k] + samples[s][k + 1:]
            got = {}
            ms["s%d_sample%d" % (s, k)] = synced(lambda: got.update(t=mc.remove_swapped_device(others, into, num, den)))
            tallies.append(got["t"].tolist())
            cleaned.append(into)
        ms["s%d_whole" % s] = sum(ms.values())
        if not keep:
            for c in cleaned:
                c.close()
        return (ms, tallies, cleaned) if keep else (ms, tallies)

    def run_merge(s):
        with counting.MoleculeCounter(nw, UL, capacity_hint=64, read_counts=True) as into:
            def go():
                for mc in samples[s]:
                    into.merge_device(mc)
            return synced(go)

    # ---- the existing calls of both libraries through the C ABI (--parent-lib), on all n reads
    vp = ctypes.c_void_p
    nf = 4096
    libs = {"this": this}
    if old:
        libs["parent"] = old
    existing = []
    if old:
        df = _features_of(di, du, nf, nf)
        o_final = torch.empty(n, dtype=torch.int64, device=dev)
        o_status = torch.empty(n, dtype=torch.uint8, device=dev)
        handles, outs = {}, {}
        for lname, lib in libs.items():
            hf, hc = vp(), vp()
            assert lib.sct_molecules_create_features(nw, nf, 3, UL, hint, 1, -1, ctypes.byref(hf)) == 0
            assert lib.sct_molecules_update_features(hf, vp(di.data_ptr()), vp(df.data_ptr()), vp(du.data_ptr()), n, None) == 0
            assert lib.sct_molecules_create_counted(nw, 3, UL, hint, ctypes.byref(hc)) == 0
            assert lib.sct_molecules_update(hc, vp(di.data_ptr()), vp(du.data_ptr()), n, None) == 0
            nm = ctypes.c_int64(0)
            tot, cap = ctypes.c_int64(0), ctypes.c_int64(0)
            assert lib.sct_molecules_info(hf, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cap)) == 0
            handles[lname] = (hf, hc)
            outs[lname] = {"collapsed": torch.empty(nw, dtype=torch.int64, device=dev),
                           "resolved": torch.empty(nw, dtype=torch.int64, device=dev),
                           "tally": torch.empty(4, dtype=torch.int64, device=dev),
                           "indptr": torch.empty(nw + 1, dtype=torch.int64, device=dev),
                           "feature": torch.empty(nm.value, dtype=torch.int32, device=dev),
                           "values": torch.empty((3, nm.value), dtype=torch.int64, device=dev), "nmol": nm.value}

        def run_update(lname, what):
            lib, h = libs[lname], vp()
            if what == "features":
                assert lib.sct_molecules_create_features(nw, nf, 3, UL, hint, 1, -1, ctypes.byref(h)) == 0
            else:
                create = lib.sct_molecules_create_counted if what == "counted" else lib.sct_molecules_create
                assert create(nw, 3, UL, hint, ctypes.byref(h)) == 0
            try:
                if what == "features":
                    return synced(lambda: lib.sct_molecules_update_features(h, vp(di.data_ptr()), vp(df.data_ptr()),
                                                                            vp(du.data_ptr()), n, None))
                return synced(lambda: lib.sct_molecules_update(h, vp(di.data_ptr()), vp(du.data_ptr()), n, None))
            finally:
                lib.sct_molecules_destroy(h)

        def run_call(lname, what):
            lib, (hf, hc), o = libs[lname], handles[lname], outs[lname]
            nnz, e, grp = ctypes.c_int64(0), vp(), vp()
            status = []
            try:
                if what == "collapse":
                    return synced(lambda: status.append(lib.sct_molecules_collapse(hf, vp(o["collapsed"].data_ptr()), None, None)))
                if what == "resolve":
                    return synced(lambda: status.append(lib.sct_molecules_resolve(
                        hf, _lib.COLLAPSE_ONE_STEP, vp(o["resolved"].data_ptr()), vp(o["tally"].data_ptr()), None)))
                if what == "matrix":
                    v = o["values"]
                    return synced(lambda: status.append(lib.sct_molecules_matrix(
                        hf, vp(o["indptr"].data_ptr()), vp(o["feature"].data_ptr()), vp(v[0].data_ptr()),
                        vp(v[1].data_ptr()), vp(v[2].data_ptr()), o["nmol"], ctypes.byref(nnz), None)))
                if what in ("merge", "downsample"):
                    assert lib.sct_molecules_create_counted(nw, 3, UL, 64, ctypes.byref(e)) == 0
                    if what == "merge":
                        return synced(lambda: status.append(lib.sct_molecules_merge(e, hc, None)))
                    return synced(lambda: status.append(lib.sct_molecules_downsample(e, hc, 2 ** 31, 0, None)))
                if what == "groups_create":
                    return synced(lambda: status.append(lib.sct_read_groups_create(hf, _lib.COLLAPSE_ONE_STEP, 0,
                                                                                   ctypes.byref(grp), None)))
                assert lib.sct_read_groups_create(hf, _lib.COLLAPSE_ONE_STEP, 0, ctypes.byref(grp), None) == 0
                return synced(lambda: status.append(lib.sct_read_groups_tag(
                    grp, vp(di.data_ptr()), vp(df.data_ptr()), vp(du.data_ptr()), n, vp(o_final.data_ptr()),
                    vp(o_status.data_ptr()), None, None, None)))
            finally:
                assert status == [0], (what, status)
                if e:
                    lib.sct_molecules_destroy(e)
                if grp:
                    lib.sct_read_groups_destroy(grp)

        existing = [("update_%s" % w, lambda lname, w=w: run_update(lname, w)) for w in ("plain", "counted", "features")]
        existing += [(w, lambda lname, w=w: run_call(lname, w))
                     for w in ("collapse", "merge", "downsample", "matrix", "resolve", "groups_create", "groups_tag")]

    # warm-up: every call once
    facts = {}
    for s in samples:
        facts[s] = run_swapped(s)[1]
        run_merge(s)
    for lname in libs:
        for _, call in existing:
            call(lname)
    rounds = []
    for r in range(args.rounds):
        row = {"what": "swapped", "round": r}
        for s in samples:
            ms, tallies = run_swapped(s)
            assert tallies == facts[s], (tallies, facts[s])  # every round: the same numbers
            row.update({k + "_ms": round(v, 3) for k, v in ms.items()})
            row["s%d_merge_ms" % s] = round(run_merge(s), 3)
        order = list(libs) if r % 2 == 0 else list(libs)[::-1]
        for what, call in existing:
            for lname in order:
                row["%s_%s_ms" % (what, lname)] = round(call(lname), 3)
        rounds.append(row)
        profile.write(json.dumps(row, sort_keys=True) + "\n")
        profile.flush()
    out = {"n": n, "nw": nw, "umi_length": UL, "hop": args.hop, "min_fraction": [num, den], "rounds": args.rounds,
           "parent_lib": bool(old), "measured": True}
    for key in rounds[0]:
        if key.endswith("_ms"):
            v = [row[key] for row in rounds]
            out[key] = {"median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
    for s in samples:
        out["s%d" % s] = {"molecules": [len(mc) for mc in samples[s]], "capacity": [mc.info()["capacity"] for mc in samples[s]],
                          "tally": facts[s]}
        out["s%d_whole_over_merge" % s] = round(out["s%d_whole_ms" % s]["median"] / out["s%d_merge_ms" % s]["median"], 3)
    if old:
        out["vs_parent"] = {what: _vs_parent(out["%s_this_ms" % what], out["%s_parent_ms" % what]) for what, _ in existing}
        out["apart_from_parent"] = sorted(what for what, v in out["vs_parent"].items() if not v["agree"])
        o, p = outs["this"], outs["parent"]
        out["abi_outputs_equal"] = bool(torch.equal(o["collapsed"], p["collapsed"]) and torch.equal(o["resolved"], p["resolved"])
                                        and torch.equal(o["tally"], p["tally"]) and torch.equal(o["indptr"], p["indptr"]))
        for lname, lib in libs.items():
            for h in handles[lname]:
                lib.sct_molecules_destroy(h)
        del outs
    # the host route, once per s, and its answers beside the device's
    umi_bits = 3 * UL
    for s in samples:
        host, tables = {}, []
        def fetch():
            for mc in samples[s]:
                index, umi, reads = mc.pairs(reads=True)
                tables.append(((index.astype(np.int64) << umi_bits) | umi.view(np.int64), reads))
        host["pairs_ms"] = round(_time_ms(fetch), 1)
        host["numpy_ms"] = round(_time_ms(lambda: host.update(a=_swapped_on_host(tables, num, den))), 1)
        answers = host.pop("a")
        host["total_ms"] = round(host["pairs_ms"] + host["numpy_ms"], 1)
        _, tallies, cleaned = run_swapped(s, keep=True)
        equal = tallies == [a[2] for a in answers]
        for mc, (keys, reads, _) in zip(cleaned, answers):
            index, umi, got = mc.pairs(reads=True)
            equal = equal and np.array_equal((index.astype(np.int64) << umi_bits) | umi.view(np.int64), keys) \
                and np.array_equal(got, reads)
            mc.close()
        host["equals_device"] = bool(equal)
        host["over_device_whole"] = round(host["total_ms"] / out["s%d_whole_ms" % s]["median"], 1)
        out["s%d_host_route_once" % s] = host
        del tables, answers
    for made in samples.values():
        for mc in made:
            mc.close()
    profile.write(json.dumps(out, sort_keys=True) + "\n")
    profile.close()
    assert all(out["s%d_host_route_once" % s]["equals_device"] for s in samples), "the device and the host route disagree"
    if old:
        assert out["abi_outputs_equal"], "an existing call's outputs differ from --parent-lib"
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process (the launcher's children)")
    ap.add_argument("--n-a", type=int, default=100_000_000, help="input A codes")
    ap.add_argument("--n-counter", type=int, default=2_000_000, help="codes given to collections.Counter")
    ap.add_argument("--n-unique", type=int, default=20_000_000, help="codes given to np.unique")
    ap.add_argument("--n-tally", type=int, default=20_000_000, help="queries of the WhitelistCorrector batch")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-collapse-host", type=int, default=200_000, help="molecules given to the dict collapse")
    ap.add_argument("--parent-lib", default="",
                    help="collapse, merge, matrix, calls, directional and downsample steps: an earlier libsctools_hip.so to time "
                         "beside this one")
    ap.add_argument("--umi-error", type=float, default=0.01,
                    help="directional step: the probability that a UMI base of a read is substituted")
    ap.add_argument("--hop", type=float, default=0.02,
                    help="resolve and groups steps: the share of the reads moved to another feature, drawn uniformly; "
                         "swapped step: the share moved to another sample")
    ap.add_argument("--only", nargs="+", choices=sorted(STEPS), help="launch only these steps")
    args = ap.parse_args()
    if args.step:
        whole = {"molecules": molecules_step, "collapse": collapse_step, "merge": merge_step, "matrix": matrix_step,
                 "calls": calls_step, "directional": directional_step, "downsample": downsample_step,
                 "resolve": resolve_step, "groups": groups_step, "swapped": swapped_step}
        if args.step in whole:
            res = whole[args.step](args)
        else:
            res = tally_step(args) if args.step == "tally" else counter_step(args.step[-1], args)
        print("RESULT " + json.dumps(res))
        return 0
    detail = {"tag": args.tag, "argv": sys.argv[1:], "steps": {}}
    rc = 0
    for step, limit in STEPS.items():
        if args.only and step not in args.only:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
               "--tag", args.tag,
               "--n-a", str(args.n_a), "--n-counter", str(args.n_counter), "--n-unique", str(args.n_unique),
               "--n-tally", str(args.n_tally), "--rounds", str(args.rounds),
               "--n-collapse-host", str(args.n_collapse_host), "--parent-lib", args.parent_lib,
               "--umi-error", str(args.umi_error), "--hop", str(args.hop)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            detail["steps"][step] = {"failed": p.returncode, "stderr": p.stderr[-2000:]}
            rc = 1
            break  # nothing more is started on the GPU after a step that failed
        detail["steps"][step] = json.loads(lines[-1][len("RESULT "):])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "count_%s.json" % args.tag)
    with open(path, "w") as f:
        json.dump(detail, f, indent=1, sort_keys=True)
        f.write("\n")
    short = {"tag": args.tag, "ok": rc == 0, "detail": os.path.relpath(path, ROOT)}
    for step, res in detail["steps"].items():
        if "device_equals_host" in res:
            short[step] = {"n": res["n"], "molecules": res["molecules"], "hop": res["hop"],
                           "device_equals_host": all(res["device_equals_host"].values()),
                           "n_shared": res["answer_one_step"]["n_shared"],
                           "ms": {k[:-3]: v["median"] for k, v in res.items() if k.endswith("_ms") and "median" in v},
                           "host_route_over_resolve": res["host_route_over_resolve"],
                           "host_route_over_matrix_resolved": res["host_route_over_matrix_resolved"]}
        elif "matrix_device_ms" in res:
            short[step] = {"n": res["n"], "nf": res["nf"], "matrix_device_ms": res["matrix_device_ms"],
                           "nnz": {k: v["nnz"] for k, v in res["matrix"].items()},
                           "host_route_ms": {k: v["host_route"]["total_ms"] for k, v in res["matrix"].items()},
                           "update_ms": {which: {k: [v[c]["median"] for c in ("plain_this_ms", "plain_features_ms",
                                                                               "counted_this_ms", "counted_features_ms")]
                                                 for k, v in modes.items()} for which, modes in res["updates"].items()}}
        elif "clusters" in res:
            short[step] = {"n": res["n"], "molecules": res["molecules"], "clusters": res["clusters"],
                           "one_step_collapsed": res["one_step_collapsed"],
                           "sweeps": res["sweeps"]["sweeps_form1"]["median"],
                           "worklist": res["worklist"],
                           "ms": {k: v["median"] for k, v in res["this"].items()}}
        elif "wave_reads_sweep_ms" in res:
            short[step] = {"n": res["n"], "molecules": res["molecules"],
                           "kept": {k: res["kept_%s" % k]["molecules"] for k in ("0.1", "0.5")},
                           "wave_reads_sweep_ms": res["wave_reads_sweep_ms"], "host_ms": res["host_route_0.5"]["total_ms"],
                           "ms": {k: v["median"] for k, v in res["downsample"].items() if "skewed" not in k},
                           "merge_ms": res["this"]["merge_ms"]["median"]}
        elif "outputs_equal" in res:
            short[step] = {"n": res["n"], "outputs_equal": all(res["outputs_equal"].values()),
                           "faster_than_parent": res["faster_than_parent"],
                           "ms": {k: [t["median"] for t in (v["this_ms"], v.get("parent_ms")) if t]
                                  for k, v in res["calls"].items()}}
        elif "reads_per_molecule" in res:
            short[step] = {"n": res["n"], "molecules": res["molecules"], "reads_per_molecule": res["reads_per_molecule"],
                           "ms": {which: {k: [v["molecules_ms"]["median"], v["counter_plus_tally_ms"]["median"]]
                                          for k, v in modes.items()} for which, modes in res["inputs"].items()}}
        elif "collapse_wave_ms" in res:
            short[step] = {"n": res["n"], "molecules": res["molecules"], "collapsed": res["collapsed"],
                           "collapse_ms": res["collapse_wave_ms"]["median"],
                           "host_ms": res["host_yardstick"]["total_scaled_ms"],
                           "ms": {which: {k: [v[c]["median"] for c in ("uncounted_ms", "counted_ms")]
                                          for k, v in modes.items()} for which, modes in res["inputs"].items()}}
        elif "host_route" in res:
            short[step] = {"n": res["n"], "molecules": res["molecules"], "host_ms": res["host_route"]["total_ms"],
                           "ms": {k: [res[k]["merge_ms"]["median"], res[k]["update_form0_src_molecules_ms"]["median"]]
                                  for k in ("plain", "counted")}}
        elif "modes" in res:
            short[step] = {"n": res["n"], "nunique": res["nunique"],
                           "ms": {k: v["median_ms"] for k, v in res["modes"].items()},
                           "host_ms": res["update_host_ms"]}
        elif "count_ms" in res:
            short[step] = {"count_ms": res["count_ms"], "nearest_plus_bincount_ms": res["nearest_plus_bincount_ms"]}
        else:
            short[step] = res
    print(json.dumps(short))
    return rc


if __name__ == "__main__":
    sys.exit(main())
