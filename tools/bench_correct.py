"""Posterior barcode correction (sct_nearest_correct) on config 4, on one box in one run.

Input: the 737,280-code whitelist, ThreeBit, in alphabetical order and shuffled, and
synthetic.config4_queries with seeded quality rows (bytes 35..74, uniform).

  query    sct_nearest_query as it is (the yardstick: with --base-lib, the same step under that
           library too, rounds interleaved, so the deferring template flag's cost to the existing
           kernel shows against the run-to-run spread)
  correct  sct_nearest_correct, device-resident: no prior (the worklist holds the distance-1 ties),
           and priors = the first pass's counts + 1 (every distance-1 query is scored); time, the
           worklist share of the queries and the share of the worklist that was accepted
  host     WhitelistCorrector.nearest / .count / .correct / .count_corrected on page-locked arrays
           against the copy time of 24 B in and 5 B out per query at the box's measured pinned copy
           rates, and the wall time per call of --calls small batches of --batch queries each (the
           fixed cost of a staged call); with --base-lib under that library too, rounds interleaved,
           and a host_verdict line: each form's median against the base's, within the base's own
           round-to-round spread or not

Every step runs in a child process of its own under its own time limit; a step that fails ends the
run.  One JSON line per step and round on stdout and in profiles/<profile>_<tag>.jsonl (--profile,
default ab_nearest_correct).

  python tools/bench_correct.py --tag mi355x [--base-lib sctools_amd/libsctools_hip_base.so]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"query": 240, "correct": 300, "host": 300}  # seconds


def _events_ms(fn, reps, torch):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return [round(t, 4) for t in out]


def _inputs(nq, torch, dev, qualities=True):
    from sctools_amd import synthetic
    n, L, seed = synthetic.CONFIGS[4]
    wl = synthetic.two_to_three(synthetic.whitelist_codes(n, L, seed), L)
    q, _, _ = synthetic.config4_queries(wl, nq, seed=4, device=dev)
    qual = None
    if qualities:
        g = torch.Generator(device=dev).manual_seed(41)
        qual = torch.randint(35, 75, (nq, L), device=dev, generator=g, dtype=torch.uint8)
    return wl, q, qual, L


def _plans(wl, L, torch, dev, stream):
    import numpy as np
    from sctools_amd import _lib
    d_wl = torch.from_numpy(wl.view(np.int64)).to(dev)
    shuf = torch.from_numpy(np.random.default_rng(7).permutation(wl.size)).to(dev)
    d_wls = d_wl[shuf].contiguous()
    torch.cuda.synchronize()
    return {"sorted": (_lib.NearestPlan(3, d_wl.data_ptr(), wl.size, 3 * L, 1, stream), d_wl),
            "shuffled": (_lib.NearestPlan(3, d_wls.data_ptr(), wl.size, 3 * L, 1, stream), d_wls)}


def _tolerate_older_library():
    """An older build (--base-lib) lacks the newest entry points: bind only what it exports."""
    import ctypes
    from sctools_amd import _lib
    path = os.environ.get("SCTOOLS_HIP_LIB")
    if not path:
        return
    rt = os.environ.get("SCTOOLS_HIP_RUNTIME") or _lib._torch_hip_runtime()
    if rt:
        ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)
    handle = ctypes.CDLL(path)
    for name in list(_lib.SIGNATURES):
        if not hasattr(handle, name):
            del _lib.SIGNATURES[name]


def query_step(args):
    import torch
    _tolerate_older_library()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    wl, q, _, L = _inputs(args.nq, torch, dev, qualities=False)
    idx = torch.empty(args.nq, dtype=torch.int32, device=dev)
    dist = torch.empty(args.nq, dtype=torch.uint8, device=dev)
    out = {"nq": args.nq, "nw": int(wl.size)}
    for name, (plan, _keep) in _plans(wl, L, torch, dev, stream).items():
        ms = _events_ms(lambda: plan.query(q.data_ptr(), args.nq, idx.data_ptr(), dist.data_ptr(), stream),
                        args.reps, torch)
        out[name + "_ms"] = ms
        out[name + "_ties_d1"] = int(((idx == -2) & (dist == 1)).sum())
        plan.close()
    return out


def correct_step(args):
    import numpy as np
    import torch
    from sctools_amd import barcode
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    wl, q, qual, L = _inputs(args.nq, torch, dev)
    nq = args.nq
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    dist = torch.empty(nq, dtype=torch.uint8, device=dev)
    ref_i, ref_d = torch.empty_like(idx), torch.empty_like(dist)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    w = barcode.phred_weights()
    out = {"nq": nq, "nw": int(wl.size), "threshold": [39, 40]}
    for name, (plan, d_wl) in _plans(wl, L, torch, dev, stream).items():
        res = {"query_ms": _events_ms(lambda: plan.query(q.data_ptr(), nq, ref_i.data_ptr(), ref_d.data_ptr(),
                                                          stream), args.reps, torch)}
        counts = torch.bincount(ref_i[ref_i >= 0].long(), minlength=wl.size)
        prior = (counts + 1).to(torch.int32).contiguous()
        for label, d_prior in (("no_prior", 0), ("prior_counts_plus_1", prior.data_ptr())):
            plan.set_posterior(d_prior, w, 39, 40, stream)
            stats.zero_()
            plan.correct(q.data_ptr(), qual.data_ptr(), L, nq, idx.data_ptr(), dist.data_ptr(), stats.data_ptr(),
                         stream)
            torch.cuda.synchronize()
            scored, accepted = (int(v) for v in stats.tolist())
            same = ~((ref_i == -2) & (ref_d == 1))
            agree = bool(torch.equal(idx[same], ref_i[same])) and bool(torch.equal(dist[same], ref_d[same]))
            ms = _events_ms(lambda: plan.correct(q.data_ptr(), qual.data_ptr(), L, nq, idx.data_ptr(),
                                                 dist.data_ptr(), 0, stream), args.reps, torch)
            res[label] = {"correct_ms": ms, "worklist": scored, "worklist_share": round(scored / nq, 6),
                          "accepted": accepted, "still_ambiguous": int((idx == -2).sum()),
                          "agrees_with_query_outside_d1_ties": agree,
                          "extra_ms_over_query": round(float(np.median(ms) - np.median(res["query_ms"])), 4)}
        out[name] = res
        plan.close()
    return out


FORMS = ("nearest", "count", "correct", "count_corrected")


def host_step(args):
    import numpy as np
    import torch
    _tolerate_older_library()
    from sctools_amd import _lib, barcode
    dev = torch.device("cuda", 0)
    nq = args.nq_host
    wl, q, qual, L = _inputs(nq, torch, dev)
    hq = _lib.pinned.empty(nq, np.uint64)
    hq[:] = q.cpu().numpy().view(np.uint64)
    hqual = _lib.pinned.empty(nq * L, np.uint8).reshape(nq, L)
    hqual[:] = qual.cpu().numpy()
    # the box's pinned copy rates, on the bytes the host form moves
    buf = torch.empty(24 * nq, dtype=torch.uint8).pin_memory()
    dbuf = torch.empty(24 * nq, dtype=torch.uint8, device=dev)
    h2d = _events_ms(lambda: dbuf.copy_(buf, non_blocking=True), args.reps, torch)
    d2h = _events_ms(lambda: buf[:5 * nq].copy_(dbuf[:5 * nq], non_blocking=True), args.reps, torch)
    del q, qual, buf, dbuf
    wc = barcode.WhitelistCorrector(wl, barcode_length=L)
    counts, _, _ = wc.count(hq)
    wc.set_prior(counts + 1)
    acc = np.zeros(wl.size, dtype=np.int64)

    def forms(a, b):
        return {"nearest": lambda: wc.nearest(hq[a:b]), "count": lambda: wc.count(hq[a:b], out=acc),
                "correct": lambda: wc.correct(hq[a:b], hqual[a:b]),
                "count_corrected": lambda: wc.count_corrected(hq[a:b], hqual[a:b], out=acc)}

    def wall(f, unit):
        t = time.perf_counter()
        f()
        return round((time.perf_counter() - t) * unit, 3)
    big = {name: [] for name in FORMS}
    whole = forms(0, nq)
    for _ in range(args.reps + 1):
        for name in FORMS:
            big[name].append(wall(whole[name], 1e3))
    share = float(wc.last_stats[0]) / nq
    # small batches, as fastq.iter_arrays hands them over: every call pays the fixed cost of the
    # staging (allocation, copies, one synchronisation), so a HIP call too many shows here
    nb, calls = args.batch, args.calls
    small = {}
    for name in FORMS:
        us = []
        for k in range(calls + 20):
            a = (k * nb) % (nq - nb)
            us.append(wall(forms(a, a + nb)[name], 1e6))
        us = np.array(us[20:])
        small[name + "_small_us"] = {"median": round(float(np.median(us)), 2), "mean": round(float(us.mean()), 2),
                                     "p90": round(float(np.percentile(us, 90)), 2)}
    wc.close()
    return {"nq": nq, **{name + "_host_ms": big[name][1:] for name in FORMS},
            "small_batch": nb, "small_calls": calls, **small,
            "worklist_share": round(share, 6),
            "copy_in_24B_per_query_ms": h2d, "copy_out_5B_per_query_ms": d2h,
            "pinned_h2d_gbs": round(24 * nq / (float(np.median(h2d)) * 1e-3) / 1e9, 2),
            "pinned_d2h_gbs": round(5 * nq / (float(np.median(d2h)) * 1e-3) / 1e9, 2)}


def host_verdict(recs):
    """Per form and batch size: the new library's median against the base's, within the base's own
    round-to-round spread (max - min of its per-round medians)?"""
    import statistics
    out = {"step": "host_verdict"}
    for name in FORMS:
        for key, pick in ((name + "_host_ms", statistics.median), (name + "_small_us", lambda v: v["median"])):
            per = {lib: [pick(r[key]) for r in recs if r["library"] == lib] for lib in ("base", "new")}
            base, new = statistics.median(per["base"]), statistics.median(per["new"])
            spread = max(per["base"]) - min(per["base"])
            out[key] = {"base_rounds": per["base"], "new_rounds": per["new"], "base": base, "new": new,
                        "base_spread": round(spread, 4), "within": abs(new - base) <= spread,
                        "slower": new - base > spread}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--step", choices=sorted(LIMITS), help="run one step in this process (the launcher's children)")
    ap.add_argument("--steps", default="query,correct,host")
    ap.add_argument("--base-lib", default=None, help="another build of the library for the A/B of the query and host steps")
    ap.add_argument("--profile", default="ab_nearest_correct", help="profiles/<profile>_<tag>.jsonl takes the lines")
    ap.add_argument("--nq", type=int, default=100_000_000)
    ap.add_argument("--nq-host", type=int, default=20_000_000)
    ap.add_argument("--batch", type=int, default=1000, help="queries per call of the host step's small batches")
    ap.add_argument("--calls", type=int, default=2000, help="small-batch calls per form")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds of the query and host steps' A/B")
    args = ap.parse_args()
    if args.step:
        res = {"query": query_step, "correct": correct_step, "host": host_step}[args.step](args)
        print("RESULT " + json.dumps(res))
        return 0
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "%s_%s.jsonl" % (args.profile, args.tag))
    runs = []
    for step in args.steps.split(","):
        if step in ("query", "host") and args.base_lib:
            libs = [("base", os.path.join(ROOT, args.base_lib)), ("new", None)]
            runs += [(step, name, lib) for _ in range(args.rounds) for name, lib in libs]
        elif step == "query":
            runs += [(step, "new", None)] * args.rounds
        else:
            runs.append((step, "new", None))
    recs = []
    with open(path, "a") as f:
        def emit(rec):
            line = json.dumps(rec, sort_keys=True)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for step, name, lib in runs:
            env = dict(os.environ)
            if lib:
                env["SCTOOLS_HIP_LIB"] = lib
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--nq", str(args.nq), "--nq-host", str(args.nq_host), "--reps", str(args.reps),
                   "--batch", str(args.batch), "--calls", str(args.calls)]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                print(json.dumps({"step": step, "library": name, "failed": p.returncode, "stderr": p.stderr[-2000:]}))
                return 1  # nothing more is started on the GPU after a step that failed
            recs.append({"tag": args.tag, "step": step, "library": name, **json.loads(lines[-1][len("RESULT "):])})
            emit(recs[-1])
        host = [r for r in recs if r["step"] == "host"]
        if args.base_lib and host:
            emit({"tag": args.tag, **host_verdict(host)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
