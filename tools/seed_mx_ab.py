"""Same-box A/B of config N's SPECTRAL seed across library builds -- the product library against the
matrix-product seed of the timing variant (sctools_amd/csrc/spectral_seed_mx.h) and its ablations:

  bash tools/build_variant_lib.sh seedmx "-DSCT_SEED_MX_VARIANT=1"
  bash tools/build_variant_lib.sh seedmx_a "-DSCT_SEED_MX_VARIANT=1 -DSCT_SEED_MX_ABL=1"
  python tools/seed_mx_ab.py walk= mx=sctools_amd/libsctools_hip_seedmx.so [--rounds 4] [--config 2]
  python tools/seed_mx_ab.py walk= mx=sctools_amd/libsctools_hip_seedmx.so --check

Each library runs in its own process, rounds interleaved; the seed and the tile are timed apart
(sct_allpairs_time_kernels: back-to-back launches over all 2^18 slices, the better of two calls).
--check instead hashes the seed bytes (sct_allpairs_seed_slices) of a few slice ranges of two small
code sets per library and fails unless every library gives the same bytes (not for ablations)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %r)
from sctools_amd import _lib, synthetic
n, L, seed = synthetic.CONFIGS[%d]
codes = synthetic.whitelist_codes(n, L, seed)
d = torch.from_numpy(codes.view(np.int64)).cuda()
p = _lib.AllPairsPlan(d.data_ptr(), n, 2 * L, scheme=_lib.SCHEME_SPECTRAL)
p.build()
c = torch.zeros(p.ncounts, dtype=torch.int64, device="cuda")
t = [p.time_kernels(c.data_ptr(), 0, p.items, repeats=10) for _ in range(2)]
print(json.dumps({"seed_ms": min(x["seed_ms"] for x in t), "tile_ms": min(x["kernel_ms"] for x in t)}))
'''
CHECK = r'''
import hashlib, json, sys
import numpy as np, torch
sys.path.insert(0, %r)
from sctools_amd import _lib, synthetic
rng = np.random.default_rng(7)
dense = (rng.choice(1 << 18, 127, replace=False).astype(np.uint64) << np.uint64(14)) | np.uint64(0x2B5C)
pair = np.concatenate([(rng.choice(1 << 18, k, replace=False).astype(np.uint64) << np.uint64(14)) | np.uint64(c)
                       for c, k in ((0x1234, 64), (0x1235, 65))])
out = {}
for name, codes in (("sparse", synthetic.whitelist_codes(5003, 16, seed=12)), ("dense", np.concatenate([dense, pair]))):
    d = torch.from_numpy(codes.view(np.int64)).cuda()
    with _lib.tuning(spectral_chunk=4096):
        p = _lib.AllPairsPlan(d.data_ptr(), codes.size, 32, scheme=_lib.SCHEME_SPECTRAL)
    p.build()
    for z0, z1 in ((0, 1), (255, 257), (777, 2277), (1000, 3600), (262143, 262144)):
        buf = torch.full(((z1 - z0) << 14,), 0x55, dtype=torch.int8, device="cuda")
        p.seed_slices(buf.data_ptr(), z0, z1)
        torch.cuda.synchronize()
        out["%%s %%d-%%d" %% (name, z0, z1)] = hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest()[:16]
    p.close()
print(json.dumps(out))
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="+", help="name=LIB (LIB relative to the repository; empty: the product library)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    child = CHECK % ROOT if a.check else TIME % (ROOT, a.config)
    res = {}
    for rnd in range(1 if a.check else a.rounds):
        for v in a.variants:
            name, lib = v.split("=", 1)
            env = dict(os.environ)
            if lib:
                env["SCTOOLS_HIP_LIB"] = os.path.join(ROOT, lib)
            out = subprocess.run([sys.executable, "-c", child], env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(json.dumps({"variant": name, "rc": out.returncode, "error": out.stderr[-800:]}), flush=True)
                return 3
            r = json.loads(out.stdout.strip().splitlines()[-1])
            print(json.dumps({"variant": name, "round": rnd, **r}), flush=True)
            res.setdefault(name, []).append(r)
    if a.check:
        first = next(iter(res.values()))[0]
        same = all(r[0] == first for r in res.values())
        print(json.dumps({"check": "bytes equal" if same else "BYTES DIFFER", "ranges": len(first)}), flush=True)
        return 0 if same else 1
    print(json.dumps({"summary": {k: {"seed_ms": [round(x["seed_ms"], 4) for x in v],
                                      "tile_ms": [round(x["tile_ms"], 4) for x in v]} for k, v in res.items()}}),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
