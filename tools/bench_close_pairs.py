"""The close-pairs pass beside the count kernel it was cut from, on one box in one run.

Input: synthetic.whitelist_codes(737280) (config 2's 16-base whitelist), device-resident, one
SUBSETS plan built once.  After clock-settle steps (untimed rounds of every call), every round runs,
interleaved: sct_allpairs_count over the whole item range, and sct_allpairs_close_pairs at
max_d = 1, 2, 3 twice each -- with room = 0 (the kernel alone: threshold, atomics on the found counter
and the degrees, no pair stored, no sort) and with room for every pair (the kernel storing its sort
words, the wait for the count, the radix sort and the unpack).  Times are device events around each
call on the null stream; the host's wall time of the full call is kept beside them.  "sort_ms" is the
full call minus the kernel-alone call of the same round: the sort, the unpack and the word stores.
One more point shows the atomic-bound end by design: a dense multiset (--dense-n codes of 4 bases,
max_d = 1, where one pair in twenty is a hit: 1e7 pairs of 2e8).

Every round is one line of profiles/ab_close_pairs.jsonl, the summary (medians, min-max spread,
ratio to the count kernel) its last; the summary is also the one JSON line on stdout.

  python tools/bench_close_pairs.py
  python tools/bench_close_pairs.py --rounds 10 --settle 3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=737280)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--dense-n", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_close_pairs.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from sctools_amd import _lib, synthetic

    dev = torch.device("cuda")

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t) * 1e3

    def bench(codes, L, max_ds, tag):
        n = codes.size
        d_codes = torch.from_numpy(codes.view(np.int64).copy()).to(dev)
        plan = _lib.AllPairsPlan(d_codes.data_ptr(), n, 2 * L, scheme=_lib.SCHEME_SUBSETS)
        plan.build()
        d_counts = torch.zeros(plan.ncounts, dtype=torch.int64, device=dev)
        d_stats = torch.zeros(6, dtype=torch.int64, device=dev)
        d_deg = torch.zeros(n * 4, dtype=torch.int32, device=dev)
        # pairs per threshold, and the room for all of them
        found = {}
        for d in max_ds:
            plan.close_pairs(d, d_stats.data_ptr())
            torch.cuda.synchronize()
            found[d] = int(d_stats[0].item())
        room = max(found.values()) + 1
        d_i = torch.empty(room, dtype=torch.int32, device=dev)
        d_j = torch.empty(room, dtype=torch.int32, device=dev)
        d_dist = torch.empty(room, dtype=torch.uint8, device=dev)

        def count():
            plan.count(d_counts.data_ptr())

        def kernel_alone(d):
            plan.close_pairs(d, d_stats.data_ptr(), d_degree_ptr=d_deg.data_ptr())

        def full(d):
            plan.close_pairs(d, d_stats.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), d_dist.data_ptr(), room,
                             d_deg.data_ptr())

        rows = []
        for r in range(-args.settle, args.rounds):  # negative rounds: clock settle, not recorded
            row = {"set": tag, "n": n, "bases": L, "round": r, "items": plan.items}
            row["count_ms"] = round(timed(count)[0], 4)
            for d in max_ds:
                k_ms, _ = timed(lambda: kernel_alone(d))
                f_ms, f_wall = timed(lambda: full(d))
                assert int(d_stats[0].item()) == found[d] == int(d_stats[1].item())
                row["max_d_%d" % d] = {"pairs": found[d], "kernel_ms": round(k_ms, 4), "full_ms": round(f_ms, 4),
                                       "full_wall_ms": round(f_wall, 4), "sort_ms": round(f_ms - k_ms, 4)}
            if r >= 0:
                rows.append(row)
        # the stored pairs are in order
        torch.cuda.synchronize()
        m = found[max_ds[-1]]
        key = (d_i[:m].to(torch.int64) << 31) | d_j[:m].to(torch.int64)
        assert m < 2 or bool((key[1:] > key[:-1]).all())
        plan.close()

        def stat(v):
            return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

        summary = {"set": tag, "n": n, "bases": L, "rounds": args.rounds, "settle": args.settle,
                   "count_ms": stat([row["count_ms"] for row in rows])}
        for d in max_ds:
            cell = {"pairs": found[d]}
            for k in ("kernel_ms", "full_ms", "full_wall_ms", "sort_ms"):
                cell[k] = stat([row["max_d_%d" % d][k] for row in rows])
            cell["kernel_over_count"] = round(cell["kernel_ms"]["median"] / summary["count_ms"]["median"], 4)
            cell["full_over_count"] = round(cell["full_ms"]["median"] / summary["count_ms"]["median"], 4)
            summary["max_d_%d" % d] = cell
        return rows, summary

    lines, out = [], {"what": "summary"}
    rows, out["whitelist"] = bench(synthetic.whitelist_codes(args.n), 16, [1, 2, 3], "whitelist")
    lines += rows
    # the atomic-bound end: a dense multiset, one pair in twenty a hit
    dense = np.random.default_rng(3).integers(0, 256, size=args.dense_n).astype(np.uint64)
    rows, out["dense"] = bench(dense, 4, [1], "dense_4_bases")
    lines += rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row, sort_keys=True) + "\n")
        f.write(json.dumps(out, sort_keys=True) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
