"""Time the GPU PCA: hlmc_pca_cov and hlmc_pca_project alone (stream events around batches of calls),
hlmc_amd.PCA.fit_transform whole (host clock, ends in a synchronise) with its host eigh share, and sklearn's PCA on the
host for orientation, at 1336 x 370 -> 32, 1336 x 290 -> 64 and 100,000 x 128 -> 32 on seeded data.

    python scripts/time_pca.py [--out FILE.json]

One process, one device; every shape is warmed up first; medians of 7 windows.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1336, 370, 32), (1336, 290, 64), (100000, 128, 32)]


def data(n, d, seed=0):
    """Gaussian rows with standard deviations 10 * 0.95^i along a seeded orthogonal basis, float32."""
    import numpy as np
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (d, d)))
    return ((rng.normal(0.0, 1.0, (n, d)) * (10.0 * 0.95 ** np.arange(d))) @ q.T).astype(np.float32)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def event_seconds(fn, calls, windows=7):
    """Median over the windows of (stream time of `calls` back-to-back calls) / calls."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / calls)
    return median(out)


def wall_seconds(fn, windows=7):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return median(out)


def shape_times(n, d, k):
    import numpy as np
    import torch
    import hlmc_amd
    from hlmc_amd import _lib as L
    from sklearn.decomposition import PCA as SkPCA
    lib = L.lib()
    X = data(n, d)
    Xd = torch.from_numpy(X).cuda()
    ws_bytes = int(lib.hlmc_pca_workspace(n, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    mean = torch.empty(d, dtype=torch.float64, device="cuda")
    G = torch.empty(d, d, dtype=torch.float64, device="cuda")
    B = torch.from_numpy(np.linalg.qr(np.random.default_rng(1).normal(size=(d, d)))[0][:, :k].copy()).cuda()
    out = torch.empty(n, k, dtype=torch.float32, device="cuda")
    calls = 200 if n < 10000 else 20
    res = {"n": n, "d": d, "k": k, "workspace_bytes": ws_bytes}
    res["cov_s"] = event_seconds(lambda: L.check(lib.hlmc_pca_cov(
        L.stream(), Xd.data_ptr(), n, d, mean.data_ptr(), G.data_ptr(), ws.data_ptr(), ws_bytes)), calls)
    res["project_s"] = event_seconds(lambda: L.check(lib.hlmc_pca_project(
        L.stream(), Xd.data_ptr(), n, d, B.data_ptr(), k, mean.data_ptr(), None, out.data_ptr())), calls)
    # algorithm counts: the upper-triangle tile pairs the kernel computes, two passes over X
    tiles = -(-d // 64)
    res["cov_fp64_flops"] = 2.0 * n * (tiles * (tiles + 1) // 2) * 64 * 64 / res["cov_s"]
    res["cov_x_bytes_per_s"] = 2.0 * n * d * 4 / res["cov_s"]
    res["project_fp64_flops"] = 2.0 * n * d * k / res["project_s"]
    model = hlmc_amd.PCA(k)
    res["fit_transform_s"] = wall_seconds(lambda: model.fit_transform(Xd))
    Gh = G.cpu().numpy()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        np.linalg.eigh(Gh)
        t.append(time.perf_counter() - t0)
    res["host_eigh_s"] = median(t)
    for solver in ("auto", "full", "covariance_eigh"):
        t = []
        for _ in range(4):
            t0 = time.perf_counter()
            SkPCA(k, svd_solver=solver, random_state=0).fit_transform(X)
            t.append(time.perf_counter() - t0)
        res[f"sklearn_{solver}_s"] = median(t[1:])
    res["host_cpus"] = len(os.sched_getaffinity(0))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_pca.py needs the GPU"
    results = []
    for n, d, k in SHAPES:
        results.append(shape_times(n, d, k))
        print(json.dumps(results[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
