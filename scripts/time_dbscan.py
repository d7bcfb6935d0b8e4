"""Time the GPU DBSCAN (DESIGN.md "DBSCAN"): a single fit at N = 20,000 and N = 100,000 and the reference's 17-radius
sweep at N = 100,000 on seeded blobs with d = 128, plus sklearn's DBSCAN at N = 20,000 on the host cores.

    python scripts/time_dbscan.py [--out FILE.json] [--steps gpu20k,gpu100k,sweep100k,sklearn20k]

Every step runs in a child process of its own under its own time limit; the first step that fails or times out ends
the run (nothing more is started on the GPU after it).  Reports wall times (median of 3 after one warm-up), the
neighbourhood pass alone (stream-timed), its fp64 FLOP/s (2 N^2 d) and the fraction of the MI355X fp64 matrix peak.
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

FP64_MATRIX_PEAK = 78.6e12   # MI355X peak fp64 matrix FLOP/s (vendor figure)
D = 128
SWEEP = [float(e) for e in range(3, 20)]
STEPS = {"gpu20k": 300, "gpu100k": 400, "sweep100k": 500, "sklearn20k": 500}   # time limits, seconds


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


def _neigh_pass_seconds(Xd, eps_list):
    """The neighbourhood pass alone (norms + distance tiles + counts), timed with stream events."""
    import ctypes as C
    import torch
    import hlmc_amd
    from hlmc_amd import _lib as L
    from hlmc_amd.cluster import _radius_sq
    lib = L.lib()
    n, d = Xd.shape
    E = len(eps_list)
    ws = torch.empty(int(lib.hlmc_dbscan_workspace(n, E)), dtype=torch.uint8, device=Xd.device)
    counts = torch.empty(E, n, dtype=torch.int32, device=Xd.device)
    border = torch.empty(E, dtype=torch.int64, device=Xd.device)
    r = (C.c_double * E)(*[_radius_sq(e) for e in eps_list])
    ts = []
    for it in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        L.check(lib.hlmc_dbscan_neighbors(L.stream(), Xd.data_ptr(), n, d, r, E, counts.data_ptr(), border.data_ptr(),
                                          ws.data_ptr(), ws.numel()), "hlmc_dbscan_neighbors")
        b.record()
        torch.cuda.synchronize()
        if it:
            ts.append(a.elapsed_time(b) * 1e-3)
    return sorted(ts)[len(ts) // 2]


def step_gpu(n, eps_list):
    import numpy as np
    import torch
    import hlmc_amd
    X = blobs(n)
    Xd = torch.from_numpy(X).cuda()
    out = {"n": n, "d": D, "radii": len(eps_list)}
    if len(eps_list) == 1:
        db = hlmc_amd.DBSCAN(eps=eps_list[0], min_samples=5)
        out["fit_s"] = _median(lambda: db.fit(Xd))
        out["clusters"] = int(db.labels_.max()) + 1
        out["noise"] = int((db.labels_ == -1).sum())
        out["borderline_pairs"] = db.n_borderline_pairs_
    else:
        res = {}
        out["sweep_s"] = _median(lambda: res.update(r=hlmc_amd.dbscan_eps_sweep(Xd, np.array(eps_list))), reps=1)
        out["best_eps"] = res["r"][0]
        out["clusters"] = [r["n_clusters"] for r in res["r"][1]]
        t0 = time.perf_counter()
        for _, _lab, _core, _b in hlmc_amd.cluster._dbscan_pass(Xd, eps_list, 5):
            pass
        torch.cuda.synchronize()
        out["sweep_without_silhouette_s"] = time.perf_counter() - t0
    t = _neigh_pass_seconds(Xd, eps_list)
    flops = 2.0 * n * n * D
    out.update(neigh_pass_s=t, neigh_fp64_flops=flops / t, neigh_fraction_of_peak=flops / t / FP64_MATRIX_PEAK)
    return out


def step_sklearn(n, eps):
    from sklearn.cluster import DBSCAN
    X = blobs(n)
    t0 = time.perf_counter()
    labels = DBSCAN(eps=eps, min_samples=5, n_jobs=16).fit_predict(X)
    return {"n": n, "d": D, "fit_s": time.perf_counter() - t0, "clusters": int(labels.max()) + 1,
            "noise": int((labels == -1).sum())}


def run_step(name):
    if name == "gpu20k":
        return step_gpu(20000, [16.0])
    if name == "gpu100k":
        return step_gpu(100000, [16.0])
    if name == "sweep100k":
        return step_gpu(100000, SWEEP)
    if name == "sklearn20k":
        return step_sklearn(20000, 16.0)
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
