"""Posterior barcode correction (sct_nearest_correct) on config 4, on one box in one run.

Input: the 737,280-code whitelist, ThreeBit, in alphabetical order and shuffled, and
synthetic.config4_queries with seeded quality rows (bytes 35..74, uniform).

  query    sct_nearest_query as it is (the yardstick: with --base-lib, the same step under that
           library too, rounds interleaved, so the deferring template flag's cost to the existing
           kernel shows against the run-to-run spread)
  correct  sct_nearest_correct, device-resident: no prior (the worklist holds the distance-1 ties),
           and priors = the first pass's counts + 1 (every distance-1 query is scored); time, the
           worklist share of the queries and the share of the worklist that was accepted
  host     WhitelistCorrector.correct / .count_corrected on page-locked arrays against the copy
           time of 24 B in and 5 B out per query at the box's measured pinned copy rates

Every step runs in a child process of its own under its own time limit; a step that fails ends the
run.  One JSON line per step and round on stdout and in profiles/ab_nearest_correct_<tag>.jsonl.

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


def host_step(args):
    import numpy as np
    import torch
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

    def wall(f):
        t = time.perf_counter()
        f()
        return round((time.perf_counter() - t) * 1e3, 3)
    t_near, t_corr, t_cnt = [], [], []
    for _ in range(args.reps + 1):
        t_near.append(wall(lambda: wc.nearest(hq)))
        t_corr.append(wall(lambda: wc.correct(hq, hqual)))
        t_cnt.append(wall(lambda: wc.count_corrected(hq, hqual)))
    share = float(wc.last_stats[0]) / nq
    wc.close()
    return {"nq": nq, "nearest_host_ms": t_near[1:], "correct_host_ms": t_corr[1:], "count_corrected_host_ms": t_cnt[1:],
            "worklist_share": round(share, 6),
            "copy_in_24B_per_query_ms": h2d, "copy_out_5B_per_query_ms": d2h,
            "pinned_h2d_gbs": round(24 * nq / (float(np.median(h2d)) * 1e-3) / 1e9, 2),
            "pinned_d2h_gbs": round(5 * nq / (float(np.median(d2h)) * 1e-3) / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--step", choices=sorted(LIMITS), help="run one step in this process (the launcher's children)")
    ap.add_argument("--steps", default="query,correct,host")
    ap.add_argument("--base-lib", default=None, help="another build of the library for the query step's A/B")
    ap.add_argument("--nq", type=int, default=100_000_000)
    ap.add_argument("--nq-host", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds of the query step")
    args = ap.parse_args()
    if args.step:
        res = {"query": query_step, "correct": correct_step, "host": host_step}[args.step](args)
        print("RESULT " + json.dumps(res))
        return 0
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "ab_nearest_correct_%s.jsonl" % args.tag)
    runs = []
    for step in args.steps.split(","):
        if step == "query":
            libs = ([("base", os.path.join(ROOT, args.base_lib))] if args.base_lib else []) + [("new", None)]
            runs += [(step, name, lib) for _ in range(args.rounds) for name, lib in libs]
        else:
            runs.append((step, "new", None))
    with open(path, "a") as f:
        for step, name, lib in runs:
            env = dict(os.environ)
            if lib:
                env["SCTOOLS_HIP_LIB"] = lib
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--nq", str(args.nq), "--nq-host", str(args.nq_host), "--reps", str(args.reps)]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                print(json.dumps({"step": step, "library": name, "failed": p.returncode, "stderr": p.stderr[-2000:]}))
                return 1  # nothing more is started on the GPU after a step that failed
            rec = {"tag": args.tag, "step": step, "library": name, **json.loads(lines[-1][len("RESULT "):])}
            line = json.dumps(rec, sort_keys=True)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
