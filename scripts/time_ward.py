"""Time the GPU Ward clustering (DESIGN.md "Ward agglomerative clustering"): the tree and the reference's 13-k sweep
(k = 2..14) at N = 1336, 8192 and 20,000 on seeded blobs with d = 128, plus sklearn's tree (one fit) and the
reference's 13-fit loop at N = 1336 and 8192 on the host.

    python scripts/time_ward.py [--out FILE.json] [--steps gpu1336,gpu8192,gpu20000,sklearn1336,sklearn8192]

Every step runs in a child process of its own under its own time limit; the first step that fails or times out ends
the run (nothing more is started on the GPU after it).  Reports wall times (median of 3 after one warm-up; one run at
N = 20,000) and the two device stages alone (stream-timed): the distance matrix with its fp64 FLOP/s (3 N^2 d / 2:
a subtract, a multiply and an add per pair of the upper triangle and k) and the chain with its time per merge.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 128
K_RANGE = range(2, 15)
STEPS = {"gpu1336": 200, "gpu8192": 200, "gpu20000": 300, "sklearn1336": 200, "sklearn8192": 500}   # limits, seconds


def blobs(n, d=D, k=10, seed=0):
    """k Gaussian blobs (std 1) around N(0, 3^2) centres, float32: latent-like data of the clustering stage."""
    import numpy as np
    rng = np.random.default_rng(seed)
    c = rng.normal(0, 3.0, (k, d))
    return (c[rng.integers(0, k, n)] + rng.normal(0, 1.0, (n, d))).astype(np.float32)


def _median(fn, reps=3):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def _stage_seconds(Xd):
    """(pdist, chain) alone, timed with stream events; the chain call ends with a stream synchronisation."""
    import torch
    from hlmc_amd import _lib as L
    lib = L.lib()
    n, d = Xd.shape
    ws_bytes = int(lib.hlmc_ward_workspace(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=Xd.device)
    ab = torch.empty(3, n - 1, dtype=torch.int32, device=Xd.device)
    md = torch.empty(n - 1, dtype=torch.float64, device=Xd.device)
    tp, tc = [], []
    for it in range(3):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        L.check(lib.hlmc_ward_pdist(L.stream(), Xd.data_ptr(), n, d, ws.data_ptr()), "hlmc_ward_pdist")
        b.record()
        L.check(lib.hlmc_ward_chain(L.stream(), n, ws.data_ptr(), ab[0].data_ptr(), ab[1].data_ptr(), md.data_ptr(),
                                    ab[2].data_ptr(), ws.data_ptr(), ws_bytes), "hlmc_ward_chain")
        c.record()
        torch.cuda.synchronize()
        if it:
            tp.append(a.elapsed_time(b) * 1e-3)
            tc.append(b.elapsed_time(c) * 1e-3)
    return min(tp), min(tc)


def step_gpu(n):
    import torch
    import hlmc_amd
    X = blobs(n)
    Xd = torch.from_numpy(X).cuda()
    reps = 3 if n <= 8192 else 1
    out = {"n": n, "d": D, "distance_matrix_bytes": n * n * 8}
    model = hlmc_amd.AgglomerativeClustering(n_clusters=10)
    out["fit_s"] = _median(lambda: model.fit(Xd), reps)
    out["cluster_sizes_k10"] = sorted(torch.bincount(torch.from_numpy(model.labels_)).tolist())
    res = {}
    out["sweep_s"] = _median(lambda: res.update(r=hlmc_amd.agglomerative_k_sweep(Xd, K_RANGE)), reps)
    out["best_k"] = res["r"][0]
    t0 = time.perf_counter()
    children, _ = hlmc_amd.cluster._ward_tree(Xd)
    t1 = time.perf_counter()
    for k in K_RANGE:
        hlmc_amd.cluster._ward_cut(children, n, k)
    out["tree_s"] = t1 - t0
    out["thirteen_cuts_s"] = time.perf_counter() - t1
    tp, tc = _stage_seconds(Xd)
    flops = 1.5 * n * n * D
    out.update(pdist_s=tp, pdist_fp64_flops=flops / tp, chain_s=tc, chain_us_per_merge=tc / (n - 1) * 1e6)
    return out


def step_sklearn(n):
    from sklearn.cluster import AgglomerativeClustering
    X = blobs(n)
    t0 = time.perf_counter()
    AgglomerativeClustering(n_clusters=10).fit_predict(X)
    t1 = time.perf_counter()
    for k in K_RANGE:       # the reference's sweep: the same tree rebuilt for every k
        AgglomerativeClustering(n_clusters=k).fit_predict(X)
    return {"n": n, "d": D, "fit_s": t1 - t0, "thirteen_fits_s": time.perf_counter() - t1}


def run_step(name):
    if name.startswith("gpu"):
        return step_gpu(int(name[3:]))
    if name.startswith("sklearn"):
        return step_sklearn(int(name[7:]))
    raise SystemExit(f"unknown step {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(run_step(args.child)), flush=True)
        return 0
    results = {}
    for name in args.steps.split(","):
        if name not in STEPS:
            raise SystemExit(f"unknown step {name}")
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True,
                               text=True, timeout=STEPS[name])
        except subprocess.TimeoutExpired:
            print(f"{name}: exceeded its {STEPS[name]} s limit; stopping", flush=True)
            results[name] = {"error": "time limit"}
            break
        line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(f"{name}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            results[name] = {"error": f"exit status {p.returncode}"}
            break
        results[name] = json.loads(line[len("RESULT "):])
        print(name, json.dumps(results[name]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 1 if any("error" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
