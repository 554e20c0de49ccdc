"""Benchmark: Hamming pair-comparisons/s, 737,280-barcode all-pairs histogram (BASELINE.json).

One step = the whole hot path of Barcodes.summarize_hamming_distances on device-resident
codes, as one rank runs it (sctools_amd.sharding.ShardedAllPairs): build the plan's
tables, count this rank's share of the work items, all-reduce the counts over RCCL
(N > 1), copy them to the host, invert them to the exact histogram, then the numpy-exact
summary.  At 737K 16-bp codes the library's AUTO scheme is SPECTRAL (the Walsh-Hadamard
route): no pair is enumerated, yet the histogram of all P = n(n-1)/2
pair distances is exact, so `value` is PAIR-EQUIVALENT throughput (P / step time, cost
independent of n).  The K timed steps run pipelined two deep (ShardedAllPairs.run, two
plans): step k+1's build runs on its own stream beside step k's count, its count is queued
before the host waits for step k's all-reduce and histogram, and every step's histogram is
produced and checked.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config 2] [--dump-outputs DIR]
  python bench.py --full [--gpus N] [--steps K] [--warmup W] [--no-paths] [--no-cpu]

A plain run does only what the headline needs: set up, settle and warm up, time the K steps,
write the last step's histogram (--dump-outputs) and print the result line.  --full adds what
takes runs of its own: the copy ceiling and the rooflines, the pair-enumerating kernel, the side
paths and the CPU baseline (the keys marked (--full) below).

--gpus N > 1 without a launcher: bench.py itself starts N rank processes (one per GPU,
backend nccl = RCCL) before anything touches a GPU, and exits non-zero if fewer than N
GPUs are visible.  Under torchrun (WORLD_SIZE set) every process is one rank and
WORLD_SIZE must equal --gpus.  Rank 0 prints one JSON line:
  value     all pairs of the whole job / max-over-ranks wall time of the K timed steps
  ranks     per-rank count / all-reduce / build / own step times
  roofline  (--full) the dominant kernel priced by HIP events recorded around every one of its
            launches in the K timed steps, on the stream the launches run on
            (sct_allpairs_timing); HBM against 8 TB/s and against a device copy measured
            in the same run; the issue-rate picture (VALU / matrix-pipe busy) from the
            committed PMC summary; the committed rocprof average beside the live one
  paths     (--full, N = 1) config 4 (100M-query nearest whitelist), config 5's 3.7M all-pairs and
            its 1e9-read encode + GC, FASTQ CB/UMI extraction, whitelist-file ingest and
            base_frequency, each timed here with its own roofline and a sampled check against
            the oracle (none of them is inside the headline's timed region)
  cpu_baseline  (--full, N = 1) the C oracle restatement (test infrastructure, never the product)
            on this host's cores, the histogram checked against the GPU's
"""

import argparse
import json
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# Full-rate VALU issue: 256 CU x 4 SIMD x 32 lanes/clk x 2.4 GHz = 78.6 T lane-slots/s
# (measured 121 lane-ops/clk/CU for v_xor_b32, profiles/valu_peak_r01.json).
VALU_PEAK_OPS = 256 * 128 * 2.4e9
L2_PEAK_BPS = 34.5e12  # aggregate L2 bandwidth, MI355X_MICROARCH.md §L2
HBM_PEAK_BPS = 8.0e12  # MI355X HBM3E (MI355X_MICROARCH.md)
SIMDS = 256 * 4
ALGO_OPS_PER_PAIR = 4  # XOR, shift-OR, AND, popcount per 32-bit code word
METRIC = "Hamming pair-comparisons/sec, 737K 10x whitelist all-pairs, 1-8 GPUs"
PROFILE_ROUND = "r06f"  # the committed rocprof / PMC summaries the line cites (profiles/)
PROFILE_FALLBACK = ("r06e", "r06", "r05", "r04")  # a kernel not re-profiled since cites its latest summary


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-steps", type=int, default=-1,
                    help="untimed steps before the warmup while the GPU clock settles (-1: 30 x world, "
                         "the same count on every rank; 0: none)")
    ap.add_argument("--config", type=int, default=2, choices=[1, 2, 3, 5])
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (the histogram) as DIR/hist.npy, float64")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: copy ceiling and rooflines, the pair "
                         "kernel, the side paths (configs 4 / 5, FASTQ, drop-in calls) and the CPU baseline")
    ap.add_argument("--cpu-seconds", type=float, default=30.0,
                    help="CPU baseline budget: the whole job if it fits, else a row sample")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-paths", action="store_true", help="--full: skip configs 4 / 5 (N = 1 paths)")
    ap.add_argument("--no-stream", action="store_true", help="--full: skip the host-resident stream paths")
    ap.add_argument("--path-steps", type=int, default=5)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL)")
    ap.add_argument("--scheme", default="auto", choices=["auto", "subsets", "moments", "spectral"])
    ap.add_argument("--pair-steps", type=int, default=5,
                    help="--full: steps of the pair-enumerating MOMENTS kernel timed beside SPECTRAL (N=1)")
    ap.add_argument("--allow-shared-gpu", action="store_true",
                    help="rehearsal only: let more ranks than GPUs share devices")
    ap.add_argument("--stub", action="store_true",
                    help="launcher test: ranks form the group and all-reduce stub counts, no GPU")
    return ap.parse_args(argv)


# ------------------------------------------------------------------ launcher
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_local_ranks(args, argv):
    """Start args.gpus rank processes of this script (RANK/LOCAL_RANK/WORLD_SIZE/MASTER_*
    set, 127.0.0.1 rendezvous), stream their output, return the worst exit code.  Runs
    before this process touches a GPU (torch.cuda.device_count() does not initialise one)."""
    n = args.gpus
    if not args.stub and args.backend == "nccl" and not args.allow_shared_gpu:
        import torch
        vis = torch.cuda.device_count()
        if vis < n:
            print("bench.py: --gpus %d but only %d GPU(s) visible; refusing to time fewer ranks" % (n, vis),
                  file=sys.stderr, flush=True)
            return 2
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0:
                    rc = rc or (code if code > 0 else 128 - code)
                    for q in pending:  # one rank failed: the others would wait in a collective
                        q.send_signal(signal.SIGTERM)
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return rc


# ------------------------------------------------------------------ CPU baseline
def _host_info():
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    return {"cpu_model": model, "nproc": os.cpu_count(), "affinity_cpus": aff, "cgroup_cpu_quota": quota,
            "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS")}


def host_threads():
    """Every host core this job may use: OMP_NUM_THREADS when the box sets the CPU share,
    else the affinity mask, capped by the cgroup quota (nproc counts the whole machine)."""
    info = _host_info()
    threads = int(info["omp_num_threads_env"] or 0) or info["affinity_cpus"] or 1
    if info["cgroup_cpu_quota"]:
        threads = max(1, min(threads, int(round(info["cgroup_cpu_quota"]))))
    return threads, info


def cpu_baseline(codes, gpu_hist, budget_s):
    """The C oracle (oracle/sct_oracle.c: encodings.py:113-121's popcount form over 32-bit
    AVX-512 lanes, OpenMP over rows) on every core this process may use: the whole job if it
    fits the budget (its histogram must equal the GPU's bin for bin), else rows [0, R)."""
    from oracle import oracle as O
    threads, info = host_threads()
    n = codes.size
    P = n * (n - 1) // 2
    rows = 2048
    t = time.perf_counter()
    _, simd = O.c_hist16(codes, 0, rows, threads=threads)
    dt = time.perf_counter() - t
    rate = (rows * (n - 1) - rows * (rows - 1) // 2) / dt
    out = {"unit": "pairs/s", "cores": threads, "kind": "port", **info,
           "kernel": "oracle_hist16 (AVX-512 VPOPCNTDQ)" if simd else "oracle_hist_popcnt (scalar popcnt)"}
    if P / rate <= budget_s:
        t = time.perf_counter()
        hist, _ = O.c_hist16(codes, threads=threads)
        dt = time.perf_counter() - t
        out.update(value=P / dt, sample="the whole job: all %d pairs of the same %d-code set in %.2f s" % (P, n, dt),
                   hist_match=bool(hist[:gpu_hist.size].tolist() == [int(x) for x in gpu_hist]
                                   and not hist[gpu_hist.size:].any()))
    else:
        rows = int(min(n - 1, max(rows, rows * budget_s / (dt * 1.2))))
        t = time.perf_counter()
        O.c_hist16(codes, 0, rows, threads=threads)
        dt = time.perf_counter() - t
        pairs = rows * (n - 1) - rows * (rows - 1) // 2
        out.update(value=pairs / dt, sample="rows [0,%d) of the same %d-code set: %d pairs in %.2f s"
                   % (rows, n, pairs, dt), hist_match=None)
    srow = 48  # the statement-for-statement loop of encodings.py:113-121, 1 core
    t = time.perf_counter()
    O.c_hist_rows(codes, 0, srow, scalar=True)
    sdt = time.perf_counter() - t
    out["scalar_1core_pairs_per_s"] = (srow * (n - 1) - srow * (srow - 1) // 2) / sdt
    out["python_reference_1core_pairs_per_s"] = 752540.0  # SURVEY.md §6, measured in the build container
    return out


# ------------------------------------------------------------------ rooflines
def _profile(name):
    """A committed PMC summary (profiles/pmc_<name>_<round>.json, tools/summarize_profile.py): this
    round's, else the latest earlier one."""
    for rnd in (PROFILE_ROUND,) + PROFILE_FALLBACK:
        path = os.path.join(ROOT, "profiles", "pmc_%s_%s.json" % (name, rnd))
        if os.path.exists(path):
            with open(path) as f:
                return dict(json.load(f), file=os.path.relpath(path, ROOT))
    return None


def _pmc_traffic(names, algo_per_unit):
    """The committed PMC summaries of a path's kernels (_profile): HBM bytes per unit of each, their
    sum and its ratio to the path's algorithmic bytes per unit (the 'traffic' of a side path)."""
    ks = {}
    for name in names:
        pr = _profile(name)
        if pr:
            ks[name] = {k: pr.get(k) for k in ("file", "trace_avg_ns", "hbm_bytes_per_unit", "valu_busy_frac")}
    if not ks or any(v["hbm_bytes_per_unit"] is None for v in ks.values()):
        return None
    tot = sum(v["hbm_bytes_per_unit"] for v in ks.values())
    return {"kernels": ks, "bytes_per_unit": tot, "vs_algorithmic": tot / algo_per_unit}


def _rocprof_avg_ms(kernel_substr, stats="kernel_stats"):
    """Average dispatch duration of a kernel in the committed rocprofv3 kernel trace of this
    bench command: over the timed steps' dispatches (profiles/<round>_timed_dispatches.json,
    the launches the live HIP events time) when present, else the --stats average of every
    dispatch (profiles/<round>_<stats>.csv: the bench command's, or config5_kernel_stats for
    config 5's path run alone); the latest round holding one.  (ms, calls, the profiled run's own
    live-vs-trace ratio, round) or Nones."""
    import csv
    for rnd in (PROFILE_ROUND,) + PROFILE_FALLBACK:
        win = os.path.join(ROOT, "profiles", "%s_timed_dispatches.json" % rnd)
        if os.path.exists(win) and stats == "kernel_stats":
            with open(win) as f:
                k = json.load(f)["kernels"].get(kernel_substr)
            if k:
                return k["avg_ns"] * 1e-6, k["window"], k.get("live_vs_trace_same_run"), rnd
        path = os.path.join(ROOT, "profiles", "%s_%s.csv" % (rnd, stats))
        if os.path.exists(path):
            with open(path) as f:
                for r in csv.DictReader(f):
                    if kernel_substr in r["Name"]:
                        return float(r["AverageNs"]) * 1e-6, int(r["Calls"]), None, rnd
    return None, None, None, None


def issue_picture(prof):
    """Issue-rate picture of one kernel from its committed PMC summary: the fraction of the
    SIMDs' cycles (at the clock the profiled run held) in which a VALU instruction is active
    (SQ_ACTIVE_INST_VALU counts quad-cycles), the matrix pipe is busy (SQ_VALU_MFMA_BUSY_CYCLES),
    and waves sit parked at s_waitcnt / barriers or stall on issue (SQ_WAIT_ANY /
    SQ_WAIT_INST_ANY over SQ_WAVE_CYCLES).  None without a profile."""
    if not prof or "pmc" not in prof:
        return None
    m, ns = prof["pmc"], prof.get("trace_avg_ns")
    out = {"source": prof["file"]}
    if "GRBM_GUI_ACTIVE" in m and ns:
        cycles = m["GRBM_GUI_ACTIVE"] / 8  # 8 XCDs
        out["clock_ghz"] = cycles / ns
        slots = SIMDS * cycles
        if "SQ_ACTIVE_INST_VALU" in m:
            out["valu_busy_frac"] = 4 * m["SQ_ACTIVE_INST_VALU"] / slots
        if "SQ_VALU_MFMA_BUSY_CYCLES" in m:
            out["mfma_busy_frac"] = m["SQ_VALU_MFMA_BUSY_CYCLES"] / slots
    if "SQ_WAVE_CYCLES" in m:
        for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"):
            if k in m:
                out[k.lower()[3:] + "_frac_of_wave_cycles"] = m[k] / m["SQ_WAVE_CYCLES"]
    if "hbm_bytes_per_launch" in prof:
        out["hbm_bytes_per_launch"] = prof["hbm_bytes_per_launch"]
    return out


def copy_ceiling_gbs(dev, mib=4096, reps=5):
    """Streaming device copy bandwidth measured in this run (sct_stream_copy: 16 B per lane,
    nontemporal, read + write bytes / time): the practical HBM ceiling the kernels are
    compared with beside the 8 TB/s spec."""
    import torch
    from sctools_amd import _lib
    a = torch.empty(mib << 20, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib = _lib.lib()
    ms = _events_ms(lambda: _lib.check(lib.sct_stream_copy(b.data_ptr(), a.data_ptr(), a.numel(), stream)), reps, dev)
    del a, b
    torch.cuda.empty_cache()
    return 2 * (mib << 20) / (ms * 1e-3) / 1e9


def spectral_roofline(kt, slices_per_launch, elem_bytes, count_ms, copy_gbs, names=("spectral_seed", "spectral"),
                      column_bits=14):
    """SPECTRAL's two kernels per chunk: seed (writes 2^14 values per virtual slice) and tile
    (reads them back: WHT over the columns + F^2 binning).  Each moves 2^14 * elem_bytes per
    virtual slice through HBM -- its algorithmic bytes -- so the HBM roofline prices both; the
    slower is reported.  column_bits 16 (dense sets, spectral16.hip): the same bytes, as 2^16
    slices of 2^16 int8 values (4 virtual slices each).  kt = {kind: (ms summed, launches)} from
    the HIP events around every launch of the timed steps."""
    algo = slices_per_launch * (1 << 14) * elem_bytes
    kern = {}
    if column_bits == 16:
        kernels = (("seed", "sct_spectral::seed16_sm_kernel (16-bit columns, int8)", names[0] + "16", "seed16_sm_kernel"),
                   ("tile", "sct_spectral::tile16_kernel (16-bit columns, int8)", names[1] + "16", "tile16_kernel"))
    else:
        kernels = (("seed", "sct_spectral::seed_sm_kernel (int8)" if elem_bytes == 1 else
                    "sct_spectral::seed_kernel<int%d_t>" % (8 * elem_bytes), names[0], "seed_sm_kernel"),
                   ("tile", "sct_spectral::tile_reg_kernel (int8 seeds)" if elem_bytes == 1
                    else "sct_spectral::tile_kernel<int%d_t>" % (8 * elem_bytes), names[1], "tile_reg_kernel"))
    for k, label, prof_name, rp in kernels:
        ms, nl = kt[k]
        avg = ms / nl if nl else float("nan")
        prof = _profile(prof_name) if elem_bytes == 1 else None
        rms, rcalls, same_run, prnd = (_rocprof_avg_ms(rp, "kernel_stats" if column_bits == 14 else "config5_kernel_stats")
                                       if elem_bytes == 1 else (None, None, None, None))
        gbs = algo / (avg * 1e-3) / 1e9
        kern[k] = {"kernel": label, "ms": avg, "launches": nl, "achieved_gbs": gbs, "frac": gbs * 1e9 / HBM_PEAK_BPS,
                   "frac_of_copy_ceiling": gbs / copy_gbs if copy_gbs else None,
                   "traffic": prof.get("hbm_bytes_per_launch") if prof else None,
                   "issue": issue_picture(prof),
                   "rocprof": None if rms is None else {
                       "avg_ms": rms, "calls": rcalls, "frac": algo / (rms * 1e-3) / HBM_PEAK_BPS,
                       "source": ("profiles/%s_timed_dispatches.json (the timed steps' dispatches of the rocprofv3 "
                                  "kernel trace of this command; every dispatch: profiles/%s_kernel_stats.csv)"
                                  % (prnd, prnd)) if column_bits == 14 else
                                 ("profiles/%s_config5_kernel_stats.csv (rocprofv3 --kernel-trace --stats of "
                                  "tools/run_paths.py config5_allpairs: every dispatch)" % prnd),
                       "live_vs_rocprof": avg / rms - 1.0,
                       "profiled_run_live_vs_rocprof": same_run,
                       "note": "live_vs_rocprof compares this run with a trace taken on another box (boxes differ "
                               "by up to ~10 %); profiled_run_live_vs_rocprof compares the profiled command's own "
                               "HIP-event time with its trace (same box, same run)"}}
    dom, other = ("seed", "tile") if kern["seed"]["ms"] >= kern["tile"]["ms"] else ("tile", "seed")
    d = kern[dom]
    return {"bound": "hbm", "achieved": d["achieved_gbs"], "peak": HBM_PEAK_BPS / 1e9, "unit": "GB/s",
            "frac": d["frac"], "traffic": d["traffic"], "kernel": d["kernel"], "kernel_ms": d["ms"],
            "launches": d["launches"], "frac_of_copy_ceiling": d["frac_of_copy_ceiling"],
            "copy_ceiling_gbs": copy_gbs, "issue": d["issue"], "rocprof": d["rocprof"],
            "other_kernel": dict(kern[other], name=other),
            "slices_per_launch": slices_per_launch, "algo_bytes_per_launch": algo,
            "count_ms_per_step": count_ms,
            "chunk_frac": 2 * algo / ((kern["seed"]["ms"] + kern["tile"]["ms"]) * 1e-3) / HBM_PEAK_BPS,
            "note": "kernel_ms: mean of HIP events recorded around every launch of this kernel in the K timed "
                    "steps, on the stream the launches run on (sct_allpairs_timing); algo bytes = the seed "
                    "values of one launch (the seed kernel writes them, the tile kernel reads them); traffic: "
                    "HBM bytes per launch from PMC (FETCH_SIZE x 2 + WRITE_SIZE, gfx950 correction); issue: "
                    "VALU / matrix-pipe busy fractions of the SIMD cycles from PMC -- neither unit is saturated, "
                    "the kernels sit between the HBM and issue ceilings (DESIGN.md §3.8); rocprof: the "
                    "committed kernel-trace average of this command, profiled (lower clock)"}


def issue_slots_per_pair(scheme):
    """VALU issue slots the bit-sliced count kernel spends per 16-bp pair, from its
    unmasked loop (v_bcnt_u32_b32 is half rate on gfx950: 2 slots)."""
    from sctools_amd import _lib
    return {_lib.SCHEME_SUBSETS: (33 + 2 * 16 + 6) / 32.0,     # nibble tables, full unroll
            _lib.SCHEME_MOMENTS: (24 + 2 * 13 + 4 + 3) / 32.0}.get(scheme, float("nan"))


def pair_roofline(job, my_pairs, kms, L):
    spp = issue_slots_per_pair(job.scheme) if L == 16 else float("nan")
    slots = my_pairs * spp / (kms * 1e-3)
    return {"bound": "valu_issue", "achieved": slots / 1e12, "peak": VALU_PEAK_OPS / 1e12,
            "unit": "T issue slots/s", "frac": slots / VALU_PEAK_OPS, "traffic": None,
            "kernel": "allpairs_count_kernel<8>", "kernel_ms": kms, "issue_slots_per_pair": spp,
            "algo_ops_per_pair": ALGO_OPS_PER_PAIR,
            "survey_ops_frac": my_pairs * ALGO_OPS_PER_PAIR / (kms * 1e-3) / VALU_PEAK_OPS,
            "note": "the bit-sliced kernel needs %.2f VALU issue slots per pair (SURVEY 8(d)'s formulation: 4 "
                    "ops); frac = issue slots used / the 78.6 T slots/s the chip offers at 2.4 GHz" % spp}


def time_pair_kernel(d_codes, L, steps):
    """The pair-enumerating MOMENTS kernel on the same codes (whole step: build, moments,
    count, inversion), for comparison with SPECTRAL."""
    import torch
    from sctools_amd import _lib, sharding
    with sharding.ShardedAllPairs(d_codes, 2 * L, _lib.SCHEME_MOMENTS) as job:
        hist = job.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            hist = job.step(timing=True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        P = job.plan.pairs
        assert int(hist.sum()) == P
        kms = job.timings()["count_ms"]
        spp = issue_slots_per_pair(job.scheme)
        return {"scheme": "moments", "value": P / dt, "unit": "pairs/s", "ms_per_step": dt * 1e3, "steps": steps,
                "kernel_ms": kms, "issue_slots_per_pair": spp,
                "issue_slot_frac": P * spp / (kms * 1e-3) / VALU_PEAK_OPS,
                "note": "enumerates every pair; issue_slot_frac is the fraction of the VALU issue slots it uses"}


# ------------------------------------------------------------------ configs 4 / 5 (N = 1)
def _events_ms(fn, reps, dev):
    import torch
    fn()
    s = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def l2_roofline(prof, nq, ms):
    """Config 4 against the L2 request ceiling: the half-key tables and the packed permutation are
    (mostly) L2-resident, so every probe is an L2 request; requests per query from the committed
    PMC pass of the query kernel (the whitelist is in key order, so the kernel writes whitelist
    indices and no index pass runs) x queries / the live time, against 34.5 TB/s of 128-B
    requests (MI355X_MICROARCH.md §L2)."""
    rq = sum((prof.get(k) or {}).get("l2_requests_per_unit") or 0.0 for k in ("nearest",))
    if not rq:
        return None
    ceil = L2_PEAK_BPS / 128.0
    rate = rq * nq / (ms * 1e-3)
    return {"requests_per_query": rq, "achieved": rate, "peak": ceil, "unit": "requests/s", "frac": rate / ceil,
            "source": [prof[k]["file"] for k in ("nearest",) if k in prof]}


def path_config4(dev, reps, copy_gbs, threads):
    """Config 4: nearest-whitelist correction of 100M ThreeBit observed barcodes against the
    737,280-code whitelist at Hamming <= 1 (sct_nearest_query on device-resident queries)."""
    import torch
    from oracle import oracle as O
    from sctools_amd import _lib, synthetic
    n, L, seed = synthetic.CONFIGS[4]
    nq = synthetic.CONFIG4_QUERIES
    wl = synthetic.two_to_three(synthetic.whitelist_codes(n, L, seed), L)
    q, pick, cls = synthetic.config4_queries(wl, nq, seed=4, device=dev)
    d_wl = torch.from_numpy(wl.view(np.int64)).to(dev)
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    dist = torch.empty(nq, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    builds = []
    for _ in range(3):  # the index build, wall-clock (its one synchronisation included); the last plan is kept
        torch.cuda.synchronize()
        t = time.perf_counter()
        plan = _lib.NearestPlan(3, d_wl.data_ptr(), n, 3 * L, 1, stream)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t) * 1e3)
        if len(builds) < 3:
            plan.close()
    build_ms = sorted(builds)[1]
    ms = _events_ms(lambda: plan.query(q.data_ptr(), nq, idx.data_ptr(), dist.data_ptr(), stream), reps, dev)
    index = plan.info()
    plan.close()
    # the same whitelist shuffled (out of alphabetical order: the index pass maps every table
    # position through the permutation): its time, and its answers equal up to the shuffle
    shuf = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)
    d_wls = d_wl[shuf].contiguous()
    plan_s = _lib.NearestPlan(3, d_wls.data_ptr(), n, 3 * L, 1, stream)
    idx_s = torch.empty_like(idx)
    dist_s = torch.empty_like(dist)
    ms_shuffled = _events_ms(lambda: plan_s.query(q.data_ptr(), nq, idx_s.data_ptr(), dist_s.data_ptr(), stream),
                             reps, dev)
    plan_s.close()
    mapped = torch.where(idx_s >= 0, shuf[idx_s.clamp(min=0).long()].int(), idx_s)
    shuffled_ok = bool(torch.equal(mapped, idx)) and bool(torch.equal(dist_s, dist))
    del d_wls, idx_s, dist_s, mapped
    torch.cuda.synchronize()  # one-shot: a fresh index and one query pass, wall-clock
    t = time.perf_counter()
    once = _lib.NearestPlan(3, d_wl.data_ptr(), n, 3 * L, 1, stream)
    once.query(q.data_ptr(), nq, idx.data_ptr(), dist.data_ptr(), stream)
    torch.cuda.synchronize()
    oneshot_ms = (time.perf_counter() - t) * 1e3
    once.close()
    exact = cls == 0
    exact_ok = bool(torch.equal(idx[exact].long(), pick[exact])) and bool((dist[exact] == 0).all())
    g = torch.Generator(device=dev).manual_seed(44)
    samp = torch.randint(0, nq, (20_000,), device=dev, generator=g)
    ridx, rdist = O.c_nearest(3, wl, q[samp].cpu().numpy().view(np.uint64), 1, threads=threads)
    sample_ok = bool(np.array_equal(idx[samp].cpu().numpy(), ridx) and np.array_equal(dist[samp].cpu().numpy(), rdist))
    algo = nq * (8 + 4 + 1)
    gbs = algo / (ms * 1e-3) / 1e9
    prof = {}
    for name in ("nearest",):
        pr = _profile(name)
        if pr:
            prof[name] = {k: pr.get(k) for k in ("file", "trace_avg_ns", "hbm_bytes_per_unit", "l2_hit_rate",
                                                   "l2_requests_per_unit", "ea_read_requests_per_unit",
                                                   "valu_busy_frac", "wait_any_frac_of_wave_cycles")}
    del q, pick, cls, idx, dist
    torch.cuda.empty_cache()
    return {"workload": "config 4: %d ThreeBit 16-bp observed barcodes (50%% exact, 25%% one substitution, "
                        "15%% one N, 10%% random) vs the %d-code whitelist, Hamming <= 1" % (nq, n),
            "value": nq / (ms * 1e-3), "unit": "queries/s", "ms": ms, "reps": reps,
            "whitelist_order": "alphabetical (as 10x ships it): the query kernel writes whitelist indices itself",
            "shuffled_whitelist_ms": ms_shuffled, "shuffled_whitelist_answers_equal": shuffled_ok,
            "index_build_ms": build_ms,
            "index_build_ms_all": builds, "build_plus_query_ms": build_ms + ms, "oneshot_build_and_query_ms": oneshot_ms,
            "index": index,
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_BPS / 1e9, "unit": "GB/s",
                         "frac": gbs * 1e9 / HBM_PEAK_BPS, "frac_of_copy_ceiling": gbs / copy_gbs,
                         "algo_bytes_per_query": 13, "kernel": "sct_nearest_query",
                         "l2": l2_roofline(prof, nq, ms),
                         "pmc": prof or None,
                         "note": "algorithmic bytes = the query stream (8 B in, 4 + 1 B out); the index "
                                 "probes are extra and mostly L2-resident: the binding ceiling is the L2 "
                                 "request rate (`l2`, DESIGN.md §3.6)"},
            "check": {"exact_draws_own_index": exact_ok, "sampled_vs_oracle": sample_ok,
                      "sample": "20,000 random queries vs oracle.c_nearest (OpenMP brute force over the whole "
                                "whitelist)"}}


def path_config5_allpairs(dev, steps, copy_gbs):
    """Config 5's all-pairs half on one GPU: 3,686,400 codes (6.79e12 pairs), SPECTRAL on 16-bit
    columns (int8 seeds; 14-bit columns would need int16), pipelined steps as the headline."""
    import torch
    from oracle import oracle as O
    from sctools_amd import _lib, sharding, synthetic
    n, L, seed = synthetic.CONFIGS[5]
    codes = synthetic.whitelist_codes(n, L, seed)
    with sharding.ShardedAllPairs(codes, 2 * L) as job:
        job.run(1)
        job.kernel_timing(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hists = job.run(steps)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        kt = job.kernel_timing(0)
        info = job.plan.spectral_info()
        roof = spectral_roofline(kt, min(info["chunk_slices"], job.end - job.begin), info["elem_bytes"], None, copy_gbs,
                                 column_bits=info["column_bits"])
        P = job.plan.pairs
    hist = hists[-1]
    ok_steps = all(np.array_equal(h, hist) for h in hists)
    m_hist = O.moments_from_hist([int(x) for x in hist], order=2)
    m_codes = O.moments_from_marginals(codes, order=2)
    return {"workload": "config 5 all-pairs: %d-code 16-bp whitelist, all %d pairs" % (n, P),
            "column_bits": info["column_bits"], "value": P / dt, "unit": "pairs/s", "ms_per_step": dt * 1e3, "steps": steps,
            "roofline": {k: roof[k] for k in ("bound", "achieved", "peak", "unit", "frac", "kernel", "kernel_ms",
                                              "launches", "frac_of_copy_ceiling", "traffic", "issue", "rocprof",
                                              "other_kernel", "algo_bytes_per_launch")},
            "check": {"steps_agree": ok_steps, "pairs": int(hist.sum()) == P,
                      "moments_vs_oracle_marginals": m_hist == m_codes,
                      "sample": "M_1, M_2 (pairs agreeing on 1 / 2 chosen positions) from the histogram vs "
                                "oracle.moments_from_marginals; the full bin-for-bin oracle check is "
                                "tests/test_gpu_parity.py::test_allpairs_config5_spectral_bin_for_bin"}}


def path_config5_encode(dev, reps, copy_gbs):
    """Config 5's read stream: 1e9 random 28-bp reads (1 % with one N) generated on the device,
    TwoBit encode + GC + flags (sct_encode) device-resident."""
    import torch
    from oracle import oracle as O
    from sctools_amd import _lib, synthetic
    n, L = synthetic.CONFIG5_READS, synthetic.CONFIG5_READ_LENGTH
    g = torch.Generator(device=dev).manual_seed(5)
    seqs = torch.randint(0, 4, (n, L), dtype=torch.uint8, device=dev, generator=g)
    chunk = 50_000_000
    for r0 in range(0, n, chunk):  # TwoBit values -> ASCII: A 65, C 67, T 84, G 71
        x = seqs[r0:r0 + chunk]
        x.copy_(65 + 2 * x + 15 * (x == 2).to(torch.uint8))
    nrows = torch.arange(0, n, 100, device=dev)
    seqs[nrows, torch.randint(0, L, (nrows.numel(),), device=dev, generator=g)] = ord("N")
    codes = torch.empty(n, dtype=torch.int64, device=dev)
    gc = torch.empty(n, dtype=torch.uint8, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run():
        _lib.check(lib.sct_encode(2, seqs.data_ptr(), n, L, L, codes.data_ptr(), gc.data_ptr(), flags.data_ptr(),
                                  stream))
    ms = _events_ms(run, reps, dev)
    torch.cuda.synchronize()
    gc_total = int(gc.sum(dtype=torch.int64))
    want_gc = sum(int((seqs[r0:r0 + chunk] == ord("C")).sum()) + int((seqs[r0:r0 + chunk] == ord("G")).sum())
                  for r0 in range(0, n, chunk))
    nflag = int(flags.sum(dtype=torch.int64))
    ok = True
    for r in range(7, n, 1_000_000):
        s = bytes(seqs[r].cpu().numpy().tobytes())
        ok = ok and int(codes[r]) == O.two_bit_encode(s) and int(gc[r]) == s.count(b"C") + s.count(b"G")
    algo = n * (L + 8 + 1 + 1)
    gbs = algo / (ms * 1e-3) / 1e9
    del seqs, codes, gc, flags
    torch.cuda.empty_cache()
    return {"workload": "config 5 read stream: %d random %d-bp reads (1%% with one N), TwoBit encode + GC + "
                        "flags, device-resident" % (n, L),
            "value": n / (ms * 1e-3), "unit": "reads/s", "ms": ms, "reps": reps,
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_BPS / 1e9, "unit": "GB/s",
                         "frac": gbs * 1e9 / HBM_PEAK_BPS, "frac_of_copy_ceiling": gbs / copy_gbs,
                         "algo_bytes_per_read": L + 10, "kernel": "encode_tiled_kernel"},
            "check": {"gc_total_vs_bytes": gc_total == want_gc, "flagged_reads": nflag == (n + 99) // 100,
                      "sampled_vs_oracle": ok,
                      "sample": "every 10^6-th read (offset 7) vs oracle.two_bit_encode; the GC total vs the C/G "
                                "bytes counted by torch; one flag per N read"}}


def _hip_runtime():
    """The HIP runtime torch loaded (for hipHostMalloc / hipHostFree from Python)."""
    import ctypes

    from sctools_amd import _lib
    rt = ctypes.CDLL(os.environ.get("SCTOOLS_HIP_RUNTIME") or _lib._torch_hip_runtime() or "libamdhip64.so")
    rt.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    rt.hipHostFree.argtypes = [ctypes.c_void_p]
    return rt


def _pinned_array(rt, shape, dtype, keep):
    """A numpy array over a fresh hipHostMalloc block (page-locked from the start, as a long-running
    ingest would allocate its buffers); the block's pointer is appended to `keep` for hipHostFree."""
    import ctypes
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = ctypes.c_void_p()
    if rt.hipHostMalloc(ctypes.byref(p), nbytes, 0) != 0 or not p.value:
        raise RuntimeError("hipHostMalloc of %d bytes failed" % nbytes)
    keep.append(p)
    buf = (ctypes.c_uint8 * nbytes).from_address(p.value)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def pcie_ceiling_gbs(dev, gib=2, reps=3):
    """Pinned host <-> device copy bandwidth measured in this run (torch copies, one direction at a
    time): the ceiling the host-resident streams are compared with."""
    import torch
    h = torch.empty(gib << 30, dtype=torch.uint8, pin_memory=True)
    d = torch.empty(gib << 30, dtype=torch.uint8, device=dev)
    h2d = _events_ms(lambda: d.copy_(h, non_blocking=True), reps, dev)
    d2h = _events_ms(lambda: h.copy_(d, non_blocking=True), reps, dev)
    del h, d
    torch.cuda.empty_cache()
    return {"h2d_gbs": (gib << 30) / (h2d * 1e-3) / 1e9, "d2h_gbs": (gib << 30) / (d2h * 1e-3) / 1e9}


def path_config5_encode_stream(dev, reps, pcie):
    """Config 5's read stream HOST-resident (SURVEY §8(d) "report both"): 1e9 28-bp reads in host
    memory (1 % with one N), TwoBit encode + GC + flags through sct_encode_stream_host (pinned,
    three stages in flight: H2D, encode, D2H), codes / GC / flags back in host memory.  The host
    buffers are page-locked allocations (hipHostMalloc, as a long-running ingest would keep them),
    which the stream copies by DMA in place."""
    import ctypes

    import torch
    from oracle import oracle as O
    from sctools_amd import _lib, synthetic
    n, L = synthetic.CONFIG5_READS, synthetic.CONFIG5_READ_LENGTH
    rt = _hip_runtime()
    blocks = []
    try:
        seqs = _pinned_array(rt, (n, L), np.uint8, blocks)
        codes = _pinned_array(rt, (n,), np.uint64, blocks)
        gc = _pinned_array(rt, (n,), np.uint8, blocks)
        flags = _pinned_array(rt, (n,), np.uint8, blocks)
        direct = all(_lib.host_pinned(a) for a in (seqs, codes, gc, flags))
        # the reads: a 2^25-read random block made on the device (ASCII A/C/G/T, one N in every 100th
        # read), copied into every block of the host array
        blk = 1 << 25
        g = torch.Generator(device=dev).manual_seed(55)
        x = torch.randint(0, 4, (blk, L), dtype=torch.uint8, device=dev, generator=g)
        x = 65 + 2 * x + 15 * (x == 2).to(torch.uint8)
        rows = torch.arange(0, blk, 100, device=dev)
        x[rows, torch.randint(0, L, (rows.numel(),), device=dev, generator=g)] = ord("N")
        hs = torch.from_numpy(seqs)
        for r0 in range(0, n, blk):
            r1 = min(n, r0 + blk)
            hs[r0:r1].copy_(x[:r1 - r0])
        torch.cuda.synchronize()
        host_block = x[:4096].cpu().numpy()
        del x
        lib = _lib.lib()

        def run():
            _lib.check(lib.sct_encode_stream_host(2, seqs.ctypes.data_as(ctypes.c_void_p), n, L,
                                                  codes.ctypes.data_as(ctypes.c_void_p),
                                                  gc.ctypes.data_as(ctypes.c_void_p),
                                                  flags.ctypes.data_as(ctypes.c_void_p), 0))
        run()  # warm: the stream's device buffers
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t)
        dt = sorted(ts)[len(ts) // 2]
        ok = bool(np.array_equal(seqs[:4096], host_block))
        for r in list(range(0, 4096, 97)) + [n - 1, n // 2 + 3, 7 * blk + 100]:
            s_ = bytes(seqs[r])
            has_n = b"N" in s_
            # an N read keeps its N as 0 with its flag set (the Python layer draws its value afterwards)
            want = O.two_bit_encode(s_.replace(b"N", b"A")) if has_n else O.two_bit_encode(s_)
            ok = ok and int(codes[r]) == want and int(gc[r]) == s_.count(b"C") + s_.count(b"G") \
                and bool(flags[r]) == has_n
        nflag = int(flags.sum(dtype=np.int64))
        want_flags = sum(len(range(0, min(blk, n - r0), 100)) for r0 in range(0, n, blk))
        del seqs, codes, gc, flags, hs
    finally:
        for p in blocks:
            rt.hipHostFree(p)
    in_bytes, out_bytes = n * L, n * 10
    gbs_in = in_bytes / dt / 1e9
    return {"workload": "config 5 read stream, host-resident: %d random %d-bp reads (1%% with one N) in host "
                        "memory -> TwoBit codes + GC + flags in host memory (sct_encode_stream_host)" % (n, L),
            "value": n / dt, "unit": "reads/s", "ms": dt * 1e3, "ms_all": [t * 1e3 for t in ts], "reps": reps,
            "roofline": {"bound": "pcie", "achieved": gbs_in, "unit": "GB/s (H2D, read bytes)",
                         "peak": pcie["h2d_gbs"], "peak_source": "pinned torch H2D copy measured in this run",
                         "frac": gbs_in / pcie["h2d_gbs"], "d2h_gbs": out_bytes / dt / 1e9,
                         "d2h_peak": pcie["d2h_gbs"],
                         "note": "%d bytes in and %d out per pass; the device side (paths.config5_encode) runs "
                                 "the same reads at HBM speed, so the host link bounds this path" % (in_bytes, out_bytes)},
            "dma_in_place": direct,
            "check": {"sampled_vs_oracle": ok, "flagged_reads": nflag == want_flags,
                      "sample": "the first 4096 reads byte for byte; 46 reads (every 97th of the first block, the "
                                "last, the middle, one N read) vs oracle.two_bit_encode (N as A), their GC and flag; one "
                                "flag per N read over all 1e9"}}


def path_host_arrays(dev, pcie, n=100_000_000, reps=3):
    """the drop-in's batch forms on HOST arrays, 100M items each --
    TwoBit.hamming_distance_array(a, b), ThreeBit.hamming_distance_array, TwoBit(16).decode_array,
    TwoBit(16).gc_content_array (encodings.py:90-121 per element) -- wall-clock per call from host
    arrays in to host arrays out.  The inputs are page-locked pool arrays (what encode_array and
    every other batch call return, _lib.pinned), so the chunked stream (include/sctools_hip.h)
    DMAs them in place; the same calls from pageable numpy copies of the inputs go through the
    library's pinned stage and its parallel host copies.  Each result is priced against the
    measured PCIe rate of its larger direction and checked against numpy on a 100K sample."""
    import torch
    from sctools_amd import _lib, encodings
    rng = np.random.default_rng(7)
    a = _lib.pinned.empty(n, np.uint64)
    b = _lib.pinned.empty(n, np.uint64)
    blk = rng.integers(0, 1 << 32, 1 << 22, dtype=np.uint64)
    for i in range(0, n, blk.size):  # (a 4M-code block repeated, its partner shifted)
        m = min(blk.size, n - i)
        a[i:i + m] = blk[:m]
        b[i:i + m] = np.roll(blk, 12345)[:m] ^ (blk[:m] & np.uint64(0xF0F0))
    samp = rng.integers(0, n, 100_000)
    x = a[samp] ^ b[samp]
    want2 = np.array([bin(int(v)).count("1") for v in ((x | (x >> np.uint64(1))) & np.uint64(0x5555555555555555))])
    want3 = np.array([bin(int(v)).count("1") for v in ((x | (x >> np.uint64(1)) | (x >> np.uint64(2)))
                                                         & np.uint64(0x9249249249249249))])
    t16 = encodings.TwoBit(16)
    want_gc = np.array([bin(int(v) & 0x55555555).count("1") for v in a[samp]])
    want_dec = [bytes(b"ACTG"[(int(v) >> (2 * (15 - p))) & 3] for p in range(16)) for v in a[samp[:2000]]]
    h2d, d2h = pcie["h2d_gbs"], pcie["d2h_gbs"]

    def timed(fn):
        fn()  # (warm: pool blocks, stage, streams)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t)
        return min(ts), r

    out = {}
    cases = (("twobit_hamming_distance_array", lambda x, y: encodings.TwoBit.hamming_distance_array(x, y),
              16, 4, lambda r: np.array_equal(r[samp], want2)),
             ("threebit_hamming_distance_array", lambda x, y: encodings.ThreeBit.hamming_distance_array(x, y),
              16, 4, lambda r: np.array_equal(r[samp], want3)),
             ("twobit_decode_array", lambda x, y: t16.decode_array(x), 8, 16,
              lambda r: [bytes(v) for v in r[samp[:2000]]] == want_dec),
             ("twobit_gc_content_array", lambda x, y: t16.gc_content_array(x), 8, 4,
              lambda r: np.array_equal(r[samp], want_gc)))
    pa, pb = np.array(a), np.array(b)  # pageable copies
    for name, fn, bin_, bout, check in cases:
        sec, r = timed(lambda: fn(a, b))
        ok = bool(check(r))
        del r
        sec_pg, r = timed(lambda: fn(pa, pb))
        ok = ok and bool(check(r))
        del r
        link = max(n * bin_ / h2d, n * bout / d2h) / 1e9  # seconds at the measured link rate
        out[name] = {"items": n, "ms": sec * 1e3, "items_per_s": n / sec, "bytes_in_per_item": bin_,
                     "bytes_out_per_item": bout, "frac_of_pcie": link / sec,
                     "pageable_inputs": {"ms": sec_pg * 1e3, "frac_of_pcie": link / sec_pg},
                     "check": {"sample_vs_numpy": ok}}
    del a, b, pa, pb
    return {"workload": "batch API on 100M host-resident items (page-locked pool arrays in, pool arrays out; "
                        "pageable numpy inputs beside)", "pcie": pcie, "calls": out,
            "note": "frac_of_pcie = (bytes of the larger direction / the measured pinned copy rate of that "
                    "direction) / wall time of the call"}


def path_fastq_stream_to_nearest(dev, threads):
    """Config 4's correction flow from FILES (VERDICT r4 missing #2): a 20M-record R1 FASTQ on the
    host's file system whose cell barcodes are config 4's observed barcodes, read lazily in pieces by
    the drop-in EmbeddedBarcodeGenerator (sct_fastq_stream_*: H2D, index, CB slices), the CBs
    ThreeBit-encoded (ThreeBit.encode_array) and corrected against the 737,280-code whitelist
    (barcode.WhitelistCorrector, built once per stream) -- host arrays between the calls, as a user of the Python API sees
    them.  Wall-clock over the whole stream (per-piece results kept as they come; joining them for
    the checks is outside the clock); the file is written (and in the page cache) before."""
    import tempfile

    import torch
    from oracle import oracle as O
    from sctools_amd import barcode, encodings, fastq, synthetic
    n, L, seed = synthetic.CONFIGS[4]
    n_rec = 20_000_000
    wl = synthetic.two_to_three(synthetic.whitelist_codes(n, L, seed), L)
    q, pick, cls = synthetic.config4_queries(wl, n_rec, seed=9, device=dev)
    three = torch.tensor(list(b"?CAGT?N?"), dtype=torch.uint8, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev).manual_seed(10)
    fd, path = tempfile.mkstemp(suffix=".fastq")
    try:
        with os.fdopen(fd, "wb") as f:
            for r0 in range(0, n_rec, 5_000_000):
                r1 = min(n_rec, r0 + 5_000_000)
                rec = torch.empty((r1 - r0, 69), dtype=torch.uint8, device=dev)
                rec[:, 0] = ord("@")
                rec[:, 1:12] = ord("r")
                rec[:, 12] = 10
                for p_ in range(L):
                    rec[:, 13 + p_] = three[(q[r0:r1] >> (3 * (L - 1 - p_))) & 7]
                rec[:, 29:39] = acgt[torch.randint(0, 4, (r1 - r0, 10), device=dev, generator=g)]
                rec[:, 39] = 10
                rec[:, 40] = ord("+")
                rec[:, 41] = 10
                rec[:, 42:68] = ord("F")
                rec[:, 68] = 10
                f.write(rec.cpu().numpy().tobytes())
                del rec
        nbytes = os.path.getsize(path)
        eb = fastq.EmbeddedBarcode(0, 16, "CR", "CY")

        parts_s = {"pieces": 0.0, "encode": 0.0, "nearest": 0.0}

        def run():
            idx_parts, dist_parts, code_parts = [], [], []
            t0 = time.perf_counter()
            corr = barcode.WhitelistCorrector(wl, max_distance=1, encoding="ThreeBit")  # (once per stream)
            parts_s["nearest"] += time.perf_counter() - t0
            gen = fastq.EmbeddedBarcodeGenerator([eb], [path], mode="rb")
            it = gen.iter_arrays(qualities=False)
            while True:
                t0 = time.perf_counter()
                arrays = next(it, None)
                t1 = time.perf_counter()
                if arrays is None:
                    parts_s["pieces"] += t1 - t0
                    break
                cb = arrays["CR"][0]
                codes = encodings.ThreeBit.encode_array(cb)
                t2 = time.perf_counter()
                idx, dist = corr.nearest(codes)
                t3 = time.perf_counter()
                parts_s["pieces"] += t1 - t0
                parts_s["encode"] += t2 - t1
                parts_s["nearest"] += t3 - t2
                idx_parts.append(idx)
                dist_parts.append(dist)
                code_parts.append(codes)
            corr.close()
            return idx_parts, dist_parts, code_parts
        run()  # warm (and the file in the page cache)
        for k in parts_s:
            parts_s[k] = 0.0
        t = time.perf_counter()
        parts = run()
        dt = time.perf_counter() - t
        # the per-piece results joined for the checks below: the checker's work, not the flow's
        # (a stream consumer handles each piece's arrays as they come)
        idx, dist, codes = (np.concatenate(p) for p in parts)
        del parts
        # the ceiling this flow runs against: the generator's own piece reader reading the same file
        # (page cache) into its page-locked buffers, nothing else
        t = time.perf_counter()
        rd = fastq._piece_reader([path], fastq.CHUNK_BYTES, fastq._HEADROOM)
        rd.start()
        try:
            while True:
                got = rd.get()
                if isinstance(got, BaseException):
                    raise got
                rd.free.put(got[0])
                if got[3]:
                    break
        finally:
            rd.close()
        read_dt = time.perf_counter() - t
    finally:
        os.unlink(path)
    qh = q.cpu().numpy().view(np.uint64)
    exact = (cls == 0).cpu().numpy()
    ok_codes = bool(np.array_equal(codes, qh))
    ok_exact = bool(np.array_equal(idx[exact], pick.cpu().numpy()[exact])) and bool((dist[exact] == 0).all())
    samp = np.random.default_rng(11).integers(0, n_rec, 20_000)
    ridx, rdist = O.c_nearest(3, wl, qh[samp], 1, threads=threads)
    ok_samp = bool(np.array_equal(idx[samp], ridx) and np.array_equal(dist[samp], rdist))
    return {"workload": "FASTQ file (%d records, %d bytes, host file system) -> EmbeddedBarcodeGenerator pieces "
                        "(sct_fastq_stream_*) -> ThreeBit.encode_array -> WhitelistCorrector.nearest vs the %d-code whitelist "
                        "at Hamming <= 1, host arrays between the calls" % (n_rec, nbytes, n),
            "value": n_rec / dt, "unit": "records/s", "ms": dt * 1e3, "file_bytes": nbytes,
            "file_gbs": nbytes / dt / 1e9, "breakdown_ms": {k: v * 1e3 for k, v in parts_s.items()},
            "roofline": {"bound": "file read", "achieved": nbytes / dt / 1e9, "unit": "GB/s of FASTQ",
                         "peak": nbytes / read_dt / 1e9, "frac": read_dt / dt,
                         "peak_source": "the same file read (page cache) by the generator's own piece reader "
                                        "(parallel positional reads into its page-locked buffers), nothing "
                                        "else, this run"},
            "note": "the drop-in Python flow end to end (file reads, four host<->device crossings per piece); "
                    "paths.fastq_to_nearest is the same work device-resident",
            "check": {"codes_equal_queries": ok_codes, "exact_draws_own_index": ok_exact,
                      "sampled_vs_oracle": ok_samp,
                      "sample": "every CB code equals the query it was printed from; every exact draw finds its own "
                                "index; 20,000 random records vs oracle.c_nearest"}}


def path_whitelist(dev, reps, copy_gbs):
    """SURVEY §8(f) ranks 1 and 4 on config 5's whitelist: the 3,686,400-line 16-bp whitelist
    file (device-resident bytes) split into `line[:-1]` records and TwoBit-encoded with GC
    (sct_lines + sct_encode_var: Barcodes.from_whitelist, barcode.py:95-97), and
    base_frequency over the codes (sct_base_frequency: barcode.py:48-70)."""
    import ctypes

    import torch
    from oracle import oracle as O
    from sctools_amd import _lib, synthetic
    n, L, seed = synthetic.CONFIGS[5]
    codes_h = synthetic.whitelist_codes(n, L, seed)
    shifts = np.arange(2 * (L - 1), -1, -2, dtype=np.uint64)
    text = np.frombuffer(b"ACTG", dtype=np.uint8)[((codes_h[:, None] >> shifts) & np.uint64(3)).astype(np.int64)]
    text = np.concatenate([text, np.full((n, 1), 10, np.uint8)], axis=1)
    buf = torch.from_numpy(text.reshape(-1)).to(dev)
    nbytes = buf.numel()
    starts = torch.empty(n, dtype=torch.int64, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    codes = torch.empty(n, dtype=torch.int64, device=dev)
    gc = torch.empty(n, dtype=torch.uint8, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    freq = torch.empty(L * 4, dtype=torch.int64, device=dev)
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    nl, mx = ctypes.c_int64(0), ctypes.c_int32(0)

    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    d_mx = torch.zeros(1, dtype=torch.int32, device=dev)

    def ingest():  # one pass, asynchronous (the count and the longest line stay on the device)
        _lib.check(lib.sct_whitelist_encode(buf.data_ptr(), nbytes, 2, 1, n, codes.data_ptr(), starts.data_ptr(),
                                            lens.data_ptr(), gc.data_ptr(), flags.data_ptr(), d_n.data_ptr(),
                                            d_mx.data_ptr(), stream))

    def basefreq():
        _lib.check(lib.sct_base_frequency(codes.data_ptr(), n, L, freq.data_ptr(), stream))
    ms_in = _events_ms(ingest, reps, dev)
    ms_bf = _events_ms(basefreq, reps, dev)
    torch.cuda.synchronize()
    nl.value, mx.value = int(d_n.item()), int(d_mx.item())
    want = torch.from_numpy(codes_h.view(np.int64)).to(dev)
    want_gc = torch.from_numpy(((text[:, :L] == ord("C")) | (text[:, :L] == ord("G"))).sum(1).astype(np.uint8)).to(dev)
    ok_in = nl.value == n and mx.value == L and torch.equal(codes, want) and torch.equal(gc, want_gc) \
        and not bool(flags.any()) and torch.equal(starts, torch.arange(n, device=dev) * (L + 1)) \
        and bool((lens == L).all())
    ok_bf = np.array_equal(freq.cpu().numpy().view(np.uint64).reshape(L, 4), O.base_frequency_numpy(codes_h, L))
    algo_in = nbytes + n * (8 + 8 + 4 + 1 + 1)
    algo_bf = 8 * n
    del buf, starts, lens, codes, gc, flags, freq
    torch.cuda.empty_cache()

    def roof(algo, ms, kernel, note):
        gbs = algo / (ms * 1e-3) / 1e9
        return {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_BPS / 1e9, "unit": "GB/s",
                "frac": gbs * 1e9 / HBM_PEAK_BPS, "frac_of_copy_ceiling": gbs / copy_gbs, "kernel": kernel,
                "note": note}
    return {"whitelist_ingest": {
                "workload": "config 5's whitelist file: %d lines of 16 bases + LF (%d bytes, device-resident): "
                            "line split (line[:-1]) + TwoBit encode + GC" % (n, nbytes),
                "value": n / (ms_in * 1e-3), "unit": "lines/s", "ms": ms_in, "reps": reps,
                "roofline": dict(roof(algo_in, ms_in, "sct_whitelist_encode (whitelist_spec16_kernel: one read of "
                                      "a file of 16-base lines; wl_count_kernel + whitelist_fused_kernel otherwise)",
                                      "algorithmic bytes: the file once + codes / starts / lens / GC / flags; 16-base "
                                      "files in one pass that also checks the layout, the count and encode passes "
                                      "returning at once (no scan launch, no host sync)"),
                                 traffic=_pmc_traffic(("whitelist_spec16",), algo_in / n)),
                "check": {"every_line": ok_in, "sample": "all %d codes, GC counts, starts and lengths vs the "
                                                         "generating codes, no flags" % n}},
            "base_frequency": {
                "workload": "base_frequency over config 5's %d 16-bp codes (device-resident)" % n,
                "value": n / (ms_bf * 1e-3), "unit": "codes/s", "ms": ms_bf, "reps": reps,
                "roofline": dict(roof(algo_bf, ms_bf, "base_frequency16_kernel (L <= 16: 32-bit SWAR) + "
                                      "base_frequency_reduce_kernel", "algorithmic bytes: the codes once"),
                                 traffic=_pmc_traffic(("base_frequency16", "base_frequency_reduce"), algo_bf / n)),
                "check": {"vs_oracle": ok_bf, "sample": "the whole table vs oracle.base_frequency_numpy"}}}


def path_dropin(dev, reps, want_summary):
    """The drop-in call itself, as a reference user makes it: Barcodes(dict of the 737,280
    config-2 codes).summarize_hamming_distances() (barcode.py:39-46), host dict in, summary dict
    out -- the key conversion, the H2D copy, the plan (probe, build, count: SPECTRAL) on the
    device's cached workspace, the exact inversion and the numpy-exact summary, wall-clock per
    call after one warm call; and the same call split into its host and device parts."""
    import torch
    from sctools_amd import _lib, barcode, synthetic
    n, L, seed = synthetic.CONFIGS[2]
    codes = synthetic.whitelist_codes(n, L, seed)
    b = barcode.Barcodes(dict.fromkeys((int(c) for c in codes), 1), L)
    first = b.summarize_hamming_distances()
    torch.cuda.synchronize()

    def timed():
        out = []
        for _ in range(reps):
            t = time.perf_counter()
            r = b.summarize_hamming_distances()
            out.append((time.perf_counter() - t) * 1e3)
        return out, r
    # the default policy (every call maps and frees its own device memory), then the opt-in
    # workspace cache (sctools_amd.keep_workspace(True): nothing mapped after the first call)
    prev = _lib.keep_workspace(False)
    free0 = torch.cuda.mem_get_info()[0]
    ts, r = timed()
    leaked = free0 - torch.cuda.mem_get_info()[0]
    _lib.keep_workspace(True)
    b.summarize_hamming_distances()
    ts_keep, r_keep = timed()
    kept = free0 - torch.cuda.mem_get_info()[0]
    parts = {"codes_array_ms": [], "hist_call_ms": [], "summary_ms": []}
    for _ in range(reps):
        t0 = time.perf_counter()
        arr = b.codes_array()
        t1 = time.perf_counter()
        h = _lib.hamming_hist_allpairs(arr, 2 * L, distinct=True)  # as hamming_histogram() calls it
        t2 = time.perf_counter()
        _lib.summary_from_hist(h)
        t3 = time.perf_counter()
        parts["codes_array_ms"].append((t1 - t0) * 1e3)
        parts["hist_call_ms"].append((t2 - t1) * 1e3)
        parts["summary_ms"].append((t3 - t2) * 1e3)
    _lib.keep_workspace(prev)
    _lib.release_plan_cache()
    med = lambda v: float(sorted(v)[len(v) // 2])  # noqa: E731
    ms = med(ts)
    P = n * (n - 1) // 2
    keys = ("minimum", "25th percentile", "median", "75th percentile", "maximum", "average")
    got = [float(r[k]) for k in keys]
    return {"workload": "Barcodes(dict of the %d config-2 codes, L=%d).summarize_hamming_distances(): host keys in, "
                        "summary dict out, one call at a time" % (n, L),
            "value": P / (ms * 1e-3), "unit": "pair-equivalents/s", "ms": ms, "ms_all": ts, "reps": reps,
            "device_bytes_left_after_calls": int(leaked),
            "keep_workspace": {"ms": med(ts_keep), "ms_all": ts_keep, "device_bytes_held": int(kept)},
            "breakdown_ms": {k: med(v) for k, v in parts.items()},
            "note": "ms: the default policy, every call maps and frees its own device memory (4 GiB transform "
                    "intermediate + codes); keep_workspace: sctools_amd.keep_workspace(True), the buffers cached "
                    "per device between calls (breakdown under this setting).  hist_call = "
                    "sct_hamming_hist_allpairs_host_ex: H2D of the codes, plan (probe + one sync), build, count "
                    "(SPECTRAL), D2H, exact inversion; codes_array = the mapping's keys -> uint64 with the "
                    "reference's type semantics (host)",
            "check": {"summary_equals_headline": (want_summary is None or got == [float(x) for x in want_summary])
                      and [float(first[k]) for k in first] == got and [float(r_keep[k]) for k in keys] == got}}


def path_scalar_calls(dev, reps=3000):
    """The reference's per-call API, one call at a time (encodings.py:75-121, 155-202): each
    TwoBit / ThreeBit scalar method in a Python loop over 256 distinct 16-bp barcodes, through the
    library's resident scalar server, median of 5 timed loops of `reps` calls;
    every answer of the first loop checked against the oracle's restatement."""
    from oracle import oracle as O
    from sctools_amd import _lib, encodings
    _lib.check(_lib.lib().sct_set_device(dev.index or 0))
    rng = np.random.default_rng(3)
    seqs = [bytes(rng.choice(list(b"ACGT"), 16).tolist()) for _ in range(256)]
    T2, T3 = encodings.TwoBit, encodings.ThreeBit
    t2 = T2(16)
    c2 = [T2.encode(x) for x in seqs]
    c3 = [T3.encode(x) for x in seqs]
    pairs2, pairs3 = list(zip(c2, c2[1:] + c2[:1])), list(zip(c3, c3[1:] + c3[:1]))
    calls = {"TwoBit.hamming_distance": (lambda k: T2.hamming_distance(*pairs2[k & 255]),
                                         lambda k: O.two_bit_hamming(*pairs2[k & 255])),
             "TwoBit.encode": (lambda k: T2.encode(seqs[k & 255]), lambda k: O.two_bit_encode(seqs[k & 255])),
             "TwoBit.decode": (lambda k: t2.decode(c2[k & 255]), lambda k: O.two_bit_decode(c2[k & 255], 16)),
             "TwoBit.gc_content": (lambda k: t2.gc_content(c2[k & 255]), lambda k: O.two_bit_gc(c2[k & 255], 16)),
             "ThreeBit.encode": (lambda k: T3.encode(seqs[k & 255]), lambda k: O.three_bit_encode(seqs[k & 255])),
             "ThreeBit.hamming_distance": (lambda k: T3.hamming_distance(*pairs3[k & 255]),
                                           lambda k: O.three_bit_hamming(*pairs3[k & 255]))}
    out, ok = {}, True
    for name, (fn, ref) in calls.items():
        ok = ok and all(fn(k) == ref(k) for k in range(256))
        loops = []
        for _ in range(5):
            t = time.perf_counter()
            for k in range(reps):
                fn(k)
            loops.append((time.perf_counter() - t) / reps * 1e6)
        out[name] = float(sorted(loops)[2])
    return {"workload": "scalar drop-in methods, one call at a time (a Python loop; 256 distinct 16-bp barcodes)",
            "unit": "us per call", "us_per_call": out,
            "reference_us_per_call": {"TwoBit.hamming_distance": 1.2, "TwoBit.encode": 2.7, "TwoBit.decode": 2.1,
                                      "TwoBit.gc_content": 1.3, "ThreeBit.encode": 2.2,
                                      "ThreeBit.hamming_distance": 1.2},
            "note": "reference: its pure-Python methods timed in the build container (SURVEY.md §6); here each "
                    "call is a PCIe round trip to the resident server wave",
            "check": {"vs_oracle": bool(ok), "sample": "256 calls of each method"}}


def _guarded(fn, *a):
    """A side path that fails reports its error in the line instead of ending the bench."""
    try:
        return fn(*a)
    except Exception as ex:  # noqa: BLE001 -- reported, never hidden
        return {"error": "%s: %s" % (type(ex).__name__, ex)}


def path_fastq(dev, reps, copy_gbs):
    """SURVEY §8(f) rank 3, the FASTQ feed: a device-resident synthetic R1 FASTQ of 20M 69-byte
    records (12-char name, 26-bp read, '+', 26 qualities), indexed (lines -> records, the '@'
    name check, fastq.py:31-38, 143-150), CB 0:16 and UMI 16:24 sequence and quality slices
    (TenXV2, fastq.py:188-200, platform.py:36-38) and the CBs TwoBit-encoded with GC."""
    import torch
    from oracle import oracle as O
    from sctools_amd import _lib
    n_rec = 20_000_000
    g = torch.Generator(device=dev).manual_seed(6)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    rec = torch.empty((n_rec, 69), dtype=torch.uint8, device=dev)
    rec[:, 0] = ord("@")
    rec[:, 1:12] = ord("r")
    rec[:, 12] = 10
    rec[:, 13:39] = acgt[torch.randint(0, 4, (n_rec, 26), device=dev, generator=g)]
    rec[:, 39] = 10
    rec[:, 40] = ord("+")
    rec[:, 41] = 10
    rec[:, 42:68] = ord("F")
    rec[:, 68] = 10
    buf = rec.reshape(-1)
    nbytes = buf.numel()
    seqs = torch.empty(n_rec * 24, dtype=torch.uint8, device=dev)  # span-major: CB rows, UMI rows
    quals = torch.empty_like(seqs)
    cb = seqs[:n_rec * 16].view(n_rec, 16)
    umi = seqs[n_rec * 16:].view(n_rec, 8)
    codes = torch.empty(n_rec, dtype=torch.int64, device=dev)
    gc = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    flags = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_ends = torch.tensor([nbytes], dtype=torch.int64, device=dev)
    status = torch.zeros(3, dtype=torch.int64, device=dev)
    spans = np.array([[0, 16], [16, 24]], dtype=np.int32)

    def run():  # one pass: index + CB / UMI slices + the CB encode, asynchronous (no host sync)
        _lib.check(lib.sct_fastq_extract_fused(
            buf.data_ptr(), nbytes, d_ends.data_ptr(), 1, 0, spans.ctypes.data, 2, n_rec, seqs.data_ptr(),
            quals.data_ptr(), None, None, codes.data_ptr(), gc.data_ptr(), flags.data_ptr(), 2, status.data_ptr(),
            stream))
    ms = _events_ms(run, reps, dev)
    i = torch.randint(0, n_rec, (256,), device=dev, generator=g)
    st = status.cpu().tolist()
    ok = st[0] == 4 * n_rec and st[1] == 0 and torch.equal(cb[i], rec[i, 13:29]) and torch.equal(umi[i], rec[i, 29:37]) \
        and torch.equal(quals[:n_rec * 16].view(n_rec, 16)[i], rec[i, 42:58]) and not bool(flags.any())
    host = cb[i].cpu().numpy()
    ok = ok and [O.two_bit_encode(bytes(r)) for r in host] == [int(x) for x in codes[i].cpu().numpy().view(np.uint64)]
    algo = nbytes + n_rec * (16 + 8) * 2 + n_rec * (8 + 1 + 1)  # FASTQ once + slices + codes / GC / flags
    gbs = algo / (ms * 1e-3) / 1e9
    del rec, buf, seqs, quals, codes, gc, flags
    torch.cuda.empty_cache()
    return {"workload": "SURVEY 8(f) rank 3: %d-record synthetic R1 FASTQ (%d bytes, device-resident): index, "
                        "CB/UMI sequence + quality slices, CB TwoBit encode + GC" % (n_rec, nbytes),
            "value": n_rec / (ms * 1e-3), "unit": "records/s", "ms": ms, "reps": reps,
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_BPS / 1e9, "unit": "GB/s",
                         "frac": gbs * 1e9 / HBM_PEAK_BPS, "frac_of_copy_ceiling": gbs / copy_gbs,
                         "algo_bytes_per_record": algo / n_rec, "kernel": "fastq_range_kernel (sct_fastq_extract_fused)",
                         "traffic": _pmc_traffic(("fastq_count", "fastq_range"), algo / n_rec),
                         "note": "algorithmic bytes: the FASTQ once + the slices + codes; a count pass, a "
                                 "one-wave reduction of the tile counts, and the extraction (contiguous tile "
                                 "ranges carrying the line numbers, the CB encode fused); no scan launch, no "
                                 "host sync (DESIGN.md §3.6)"},
            "check": {"sampled": ok, "sample": "256 random records: CB / UMI / CB-quality slices equal the "
                                               "record bytes, CB codes vs oracle.two_bit_encode"}}


def path_pipeline(dev, reps, copy_gbs, threads):
    """The correction flow end to end at size (VERDICT r3 missing #4): a device-resident R1 FASTQ
    whose 20M cell barcodes are config 4's observed barcodes (50 % whitelist draws, 25 % one
    substitution, 15 % one N, 10 % random), the CB / UMI slices (fastq.py:188-200, TenXV2
    platform.py:36-37) with the CB ThreeBit-encoded as it is sliced (N kept,
    encodings.py:155-167), then the nearest whitelist barcode at Hamming <= 1 (config 4's index
    over the 737,280-code whitelist, encodings.py:194-202).  Timed: extraction + query; the
    index is built once beside it (`index_build_ms`)."""
    import torch
    from oracle import oracle as O
    from sctools_amd import _lib, synthetic
    n, L, seed = synthetic.CONFIGS[4]
    n_rec = 20_000_000
    wl = synthetic.two_to_three(synthetic.whitelist_codes(n, L, seed), L)
    q, pick, cls = synthetic.config4_queries(wl, n_rec, seed=7, device=dev)
    g = torch.Generator(device=dev).manual_seed(8)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    three = torch.tensor(list(b"?CAGT?N?"), dtype=torch.uint8, device=dev)  # ThreeBit value -> base
    rec = torch.empty((n_rec, 69), dtype=torch.uint8, device=dev)
    rec[:, 0] = ord("@")
    rec[:, 1:12] = ord("r")
    rec[:, 12] = 10
    for p_ in range(L):  # the CB: the query's bases, MSB-first
        rec[:, 13 + p_] = three[(q >> (3 * (L - 1 - p_))) & 7]
    rec[:, 29:39] = acgt[torch.randint(0, 4, (n_rec, 10), device=dev, generator=g)]
    rec[:, 39] = 10
    rec[:, 40] = ord("+")
    rec[:, 41] = 10
    rec[:, 42:68] = ord("F")
    rec[:, 68] = 10
    buf = rec.reshape(-1)
    nbytes = buf.numel()
    seqs = torch.empty(n_rec * 24, dtype=torch.uint8, device=dev)
    quals = torch.empty_like(seqs)
    codes = torch.empty(n_rec, dtype=torch.int64, device=dev)
    flags = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    idx = torch.empty(n_rec, dtype=torch.int32, device=dev)
    dist = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_ends = torch.tensor([nbytes], dtype=torch.int64, device=dev)
    status = torch.zeros(3, dtype=torch.int64, device=dev)
    spans = np.array([[0, 16], [16, 24]], dtype=np.int32)
    d_wl = torch.from_numpy(wl.view(np.int64)).to(dev)
    for k in range(2):  # the second build is the one reported (the first pays the first-use costs)
        torch.cuda.synchronize()
        t = time.perf_counter()
        plan = _lib.NearestPlan(3, d_wl.data_ptr(), n, 3 * L, 1, stream)
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t) * 1e3
        if k == 0:
            plan.close()

    def extract():
        _lib.check(lib.sct_fastq_extract_fused(
            buf.data_ptr(), nbytes, d_ends.data_ptr(), 1, 0, spans.ctypes.data, 2, n_rec, seqs.data_ptr(),
            quals.data_ptr(), None, None, codes.data_ptr(), None, flags.data_ptr(), 3, status.data_ptr(), stream))

    def query():
        plan.query(codes.data_ptr(), n_rec, idx.data_ptr(), dist.data_ptr(), stream)

    def run():
        extract()
        query()
    ms = _events_ms(run, reps, dev)
    ms_x = _events_ms(extract, reps, dev)
    ms_q = _events_ms(query, reps, dev)
    plan.close()
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    ok_codes = st[0] == 4 * n_rec and st[1] == 0 and bool(torch.equal(codes, q)) and not bool(flags.any())
    exact = cls == 0
    ok_exact = bool(torch.equal(idx[exact].long(), pick[exact])) and bool((dist[exact] == 0).all())
    samp = torch.randint(0, n_rec, (20_000,), device=dev, generator=g)
    ridx, rdist = O.c_nearest(3, wl, q[samp].cpu().numpy().view(np.uint64), 1, threads=threads)
    ok_samp = bool(np.array_equal(idx[samp].cpu().numpy(), ridx) and np.array_equal(dist[samp].cpu().numpy(), rdist))
    algo = nbytes + n_rec * (16 + 8) * 2 + n_rec * (8 + 1) + n_rec * (8 + 4 + 1)
    gbs = algo / (ms * 1e-3) / 1e9
    del rec, buf, seqs, quals, codes, flags, idx, dist, q, pick, cls
    torch.cuda.empty_cache()
    return {"workload": "FASTQ -> CB ThreeBit -> nearest whitelist at size: %d-record R1 FASTQ (%d bytes, "
                        "device-resident) whose CBs are config 4's observed barcodes, vs the %d-code "
                        "whitelist at Hamming <= 1" % (n_rec, nbytes, n),
            "value": n_rec / (ms * 1e-3), "unit": "records/s", "ms": ms, "reps": reps,
            "extract_ms": ms_x, "query_ms": ms_q, "index_build_ms": build_ms,
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_BPS / 1e9, "unit": "GB/s",
                         "frac": gbs * 1e9 / HBM_PEAK_BPS, "frac_of_copy_ceiling": gbs / copy_gbs,
                         "algo_bytes_per_record": algo / n_rec,
                         "kernel": "fastq_range_kernel (ThreeBit CB fused) + halves_query_kernel",
                         "note": "algorithmic bytes: the FASTQ once + slices + codes / flags written, the "
                                 "codes read again by the query + index / distance written"},
            "check": {"codes_equal_queries": ok_codes, "exact_draws_own_index": ok_exact,
                      "sampled_vs_oracle": ok_samp,
                      "sample": "every CB code equals the query it was printed from; every exact draw finds "
                                "its own index; 20,000 random records vs oracle.c_nearest"}}


# ------------------------------------------------------------------ ranks
def run_stub(args, rank, world):
    """Launcher check without a GPU: the ranks form a gloo group and all-reduce stub counts
    (rank r contributes (r + 1) * [0, 1, ..., 17]) `steps` times."""
    import torch
    import torch.distributed as dist
    dist.init_process_group(args.backend, rank=rank, world_size=world)
    try:
        base = torch.arange(18, dtype=torch.int64)
        want = base * (world * (world + 1) // 2)
        ok = True
        t0 = time.perf_counter()
        for _ in range(args.warmup + args.steps):
            c = base * (rank + 1)
            dist.all_reduce(c)
            ok = ok and torch.equal(c, want)
        dt = time.perf_counter() - t0
        flags = torch.tensor([int(ok), rank], dtype=torch.int64)
        allf = [torch.zeros_like(flags) for _ in range(world)]
        dist.all_gather(allf, flags)
        if rank == 0:
            print(json.dumps({"stub": True, "n_gpus": dist.get_world_size(), "backend": dist.get_backend(),
                              "ranks_seen": sorted(int(f[1]) for f in allf),
                              "allreduce_ok": all(int(f[0]) for f in allf), "steps": args.steps,
                              "warmup": args.warmup, "seconds": dt}), flush=True)
    finally:
        dist.destroy_process_group()
    return 0


def run_rank(args, rank, world, local):
    import torch
    import torch.distributed as dist
    from sctools_amd import _lib, sharding, synthetic

    ndev = torch.cuda.device_count()
    if local >= ndev and not args.allow_shared_gpu:
        print("bench.py: rank %d (local %d) has no GPU of its own (%d visible)" % (rank, local, ndev),
              file=sys.stderr, flush=True)
        return 2
    dev_index = local % max(1, ndev)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    backend = dist.get_backend() if world > 1 else None
    _lib.check(_lib.lib().sct_set_device(dev_index))

    n, L, seed = synthetic.CONFIGS[args.config]
    codes = synthetic.whitelist_codes(n, L, seed)
    scheme = {"auto": _lib.SCHEME_AUTO, "subsets": _lib.SCHEME_SUBSETS, "moments": _lib.SCHEME_MOMENTS,
              "spectral": _lib.SCHEME_SPECTRAL}[args.scheme]
    job = sharding.ShardedAllPairs(codes, 2 * L, scheme)
    spectral = job.scheme == _lib.SCHEME_SPECTRAL
    # steps run software-pipelined two deep (ShardedAllPairs.run): every step's zero, build,
    # count, all-reduce, read-back and inversion happen inside the timed region; step k+1's
    # kernels are queued before the host waits for step k's histogram
    # The GPU clock settles over the first ~40 ms of a fresh box's load (rocprof traces: the tile
    # kernel runs 1.51 ms on the 3rd launch and 1.07 from the ~20th): untimed steps first, a fixed
    # count on every rank (each step holds a collective), then the W warmup steps
    settle = 30 * world if args.settle_steps < 0 else args.settle_steps
    if settle:
        job.run(settle)
    job.run(args.warmup)
    job.reset_timings()  # the timings cover the timed steps only
    job.kernel_timing(1)  # HIP events around every kernel launch of the timed steps
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hists = job.run(args.steps, timing=True)
    torch.cuda.synchronize()
    mine = time.perf_counter() - t0  # this rank's own wall time, before waiting for the others
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    kt = job.kernel_timing(0)
    tm = job.timings()
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        row = torch.tensor([rank, tm["count_ms"], tm["allreduce_us"], tm["build_ms"], mine * 1e3 / args.steps,
                            job.end - job.begin], dtype=torch.float64, device=dev)
        rows = [torch.zeros_like(row) for _ in range(world)]
        dist.all_gather(rows, row)
        per_rank = [dict(zip(("rank", "count_ms", "allreduce_us", "build_ms", "step_ms", "items"),
                             [float(v) for v in r.cpu().tolist()])) for r in rows]
    else:
        per_rank = [{"rank": 0, "count_ms": tm["count_ms"], "allreduce_us": None, "build_ms": tm["build_ms"],
                     "step_ms": mine * 1e3 / args.steps, "items": job.end - job.begin}]
    for r in per_rank:
        r["rank"], r["items"] = int(r["rank"]), int(r["items"])

    hist = hists[-1]
    assert len(hists) == args.steps and all(np.array_equal(h, hist) for h in hists), "steps disagree"
    P = job.plan.pairs
    assert int(hist.sum()) == P, "histogram does not cover every pair"
    summ = _lib.summary_from_hist(hist)
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: the exact histogram
        # (counts below 2^53, so float64 holds them exactly); the codes are seeded, so two
        # builds given the same arguments can be compared bin for bin
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "hist.npy"), hist.astype(np.float64))
    copy_gbs = roofline = pair_kernel = None
    if args.full:
        copy_gbs = copy_ceiling_gbs(dev) if rank == 0 else None
        if spectral:
            info = job.plan.spectral_info()
            roofline = spectral_roofline(kt, min(info["chunk_slices"], job.end - job.begin), info["elem_bytes"],
                                         tm["count_ms"], copy_gbs, column_bits=info["column_bits"])
        else:
            roofline = pair_roofline(job, job.my_pairs(), kt["count"][0] / max(1, kt["count"][1]), L)
        if spectral and world == 1 and args.pair_steps > 0:
            pair_kernel = time_pair_kernel(job.d_codes, L, args.pair_steps)
    job.close()

    out = None
    if rank == 0:
        out = {
            "metric": METRIC,
            "value": P * args.steps / elapsed,
            "unit": "pairs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "settle_steps": settle,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "i32" if spectral else "u32",
            "data": "synthetic (seeded uniform random unique 16-bp codes, sctools_amd/synthetic.py)",
            "config": {"workload": "config %d: %d-barcode all-pairs TwoBit Hamming histogram + summary"
                                   % (args.config, n),
                       "barcodes": n, "barcode_length": L, "pairs": P,
                       "scheme": {0: "subsets", 1: "moments", 2: "spectral"}[job.scheme],
                       "value_kind": ("pair-equivalent: the exact histogram of all P pairs from a Walsh-Hadamard "
                                      "transform that enumerates no pair (cost independent of n)") if spectral
                       else "enumerated pairs",
                       "parallelism": ("%d ranks, %s; %s all-reduce of %d int64 counts" % (
                           world, "transform-slice shards" if spectral else "item-range + moment shards",
                           "RCCL" if backend == "nccl" else str(backend), job.plan.ncounts))
                       if world > 1 else "single GPU",
                       "backend": backend},
            "ranks": per_rank,
            "roofline": roofline,
            "summary": dict(zip(("minimum", "p25", "median", "p75", "maximum", "average"),
                                [float(x) for x in summ])),
            "hist": [int(x) for x in hist],
        }
        if not args.full:
            del out["roofline"]
        if pair_kernel is not None:
            out["pair_kernel"] = pair_kernel
    if rank == 0 and world == 1 and args.full:
        threads, _ = host_threads()
        if not args.no_paths:
            # configs 4 and 5 (BASELINE.json), each timed on its own after the headline
            out["paths"] = {"config4_nearest": path_config4(dev, args.path_steps, copy_gbs, threads),
                            "config5_allpairs": path_config5_allpairs(dev, max(2, args.path_steps), copy_gbs),
                            "config5_encode": path_config5_encode(dev, max(2, args.path_steps // 2), copy_gbs),
                            "fastq_ingest": _guarded(path_fastq, dev, max(2, args.path_steps), copy_gbs),
                            "fastq_to_nearest": _guarded(path_pipeline, dev, max(2, args.path_steps), copy_gbs,
                                                         threads)}
            wl = _guarded(path_whitelist, dev, max(5, args.path_steps), copy_gbs)
            out["paths"].update(wl if "error" not in wl else {"whitelist_ingest": wl})
            if not args.no_stream:  # host-resident streams (SURVEY §8(d) "report both")
                pcie = _guarded(pcie_ceiling_gbs, dev)
                out["paths"]["pcie_ceiling"] = pcie
                if "error" not in pcie:
                    out["paths"]["config5_encode_stream"] = _guarded(path_config5_encode_stream, dev, 2, pcie)
                    out["paths"]["host_arrays"] = _guarded(path_host_arrays, dev, pcie)
                out["paths"]["fastq_stream_to_nearest"] = _guarded(path_fastq_stream_to_nearest, dev, threads)
            if args.config == 2:
                out["paths"]["dropin_summary_737k"] = _guarded(path_dropin, dev, max(5, args.path_steps), summ)
            out["paths"]["scalar_calls"] = _guarded(path_scalar_calls, dev)
        if not args.no_cpu:
            out["cpu_baseline"] = cpu_baseline(codes, hist, args.cpu_seconds)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None:
        if args.gpus > 1:
            return launch_local_ranks(args, argv)
        world, rank, local = 1, 0, 0
    else:
        world = int(env_world)
        rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", str(rank)))
        if world != args.gpus:
            print("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world), file=sys.stderr, flush=True)
            return 2
    if args.stub:
        return run_stub(args, rank, world)
    return run_rank(args, rank, world, local)


if __name__ == "__main__":
    sys.exit(main())
