"""Time the GPU t-SNE: hlmc_tsne_knn, hlmc_tsne_affinities and one hlmc_tsne_gradient alone (stream
events around batches of calls), one iteration of hlmc_tsne_run (events around a 50-iteration call), and
hlmc_amd.TSNE.fit_transform whole (host clock, ends in a synchronise), at 1336 x 32, 1336 x 64 and 100,000 x 128 on
seeded blobs; sklearn 1.7.2's TSNE on the host (16 threads) at the two small shapes for orientation.

    python scripts/time_tsne.py [--out FILE.json] [--shapes small|large|all] [--sklearn]

One process, one device; every shape is warmed up first; medians of 5 windows (1 window of the large shape's fit).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL = [(1336, 32, 6), (1336, 64, 6)]
LARGE = [(100000, 128, 10)]


def data(n, d, centres, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    C = rng.normal(0.0, 1.0, (centres, d)) * 10.0
    return (C[np.arange(n) % centres] + rng.normal(0.0, 1.0, (n, d))).astype(np.float32)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def event_seconds(fn, calls, windows=5, warm=1):
    import torch
    for _ in range(warm):
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


def time_shape(n, d, centres, dev):
    import numpy as np
    import torch
    import hlmc_amd
    from hlmc_amd import _lib as L
    from hlmc_amd import manifold as M
    lib = L.lib()
    big = n > 20000
    Xd = torch.as_tensor(data(n, d, centres), device=dev)
    aff = M.Affinities(Xd, 30.0)
    torch.cuda.synchronize()
    k = aff.k

    def knn():
        L.check(lib.hlmc_tsne_knn(L.stream(), Xd.data_ptr(), n, d, k, aff.nbr_idx.data_ptr(), aff.nbr_d2.data_ptr(),
                                  aff.ws.data_ptr(), aff.ws_bytes))

    def affinities():
        L.check(lib.hlmc_tsne_affinities(L.stream(), aff.nbr_idx.data_ptr(), aff.nbr_d2.data_ptr(), n, k, 30.0,
                                         aff.beta.data_ptr(), aff.cond_p.data_ptr(), aff.indptr.data_ptr(),
                                         aff.indices.data_ptr(), aff.values.data_ptr(), aff.ws.data_ptr(),
                                         aff.ws_bytes))

    Y0 = (np.random.RandomState(0).standard_normal((n, 2)) * 10.0).astype(np.float32)     # a spread-out embedding
    state = M.Descent(aff, Y0)
    grad = torch.empty(n, 2, dtype=torch.float32, device=dev)

    def gradient():
        L.check(lib.hlmc_tsne_gradient(L.stream(), state.Y.data_ptr(), n, aff.indptr.data_ptr(), aff.indices.data_ptr(),
                                       aff.values.data_ptr(), 1.0, grad.data_ptr(), state.stats.data_ptr(), 1,
                                       aff.ws.data_ptr(), aff.ws_bytes))

    iters = 10 if big else 50

    def run_chunk():
        state._run(iters, 1.0, 0.8, 200.0)

    rec = dict(n=n, d=d, k=k, nnz=int(aff.indptr[-1].item()))
    rec["knn_s"] = event_seconds(knn, 1 if big else 20, windows=3 if big else 5)
    rec["affinities_s"] = event_seconds(affinities, 1 if big else 20, windows=3 if big else 5)
    rec["gradient_s"] = event_seconds(gradient, 5 if big else 100)
    rec["iteration_s"] = event_seconds(run_chunk, 1, windows=3 if big else 5) / iters
    rec["pairs_per_s"] = n * (n - 1.0) / rec["gradient_s"]

    def fit():
        hlmc_amd.TSNE(random_state=42, device=dev).fit_transform(Xd)
        torch.cuda.synchronize()

    if not big:
        fit()
    out = []
    for _ in range(1 if big else 5):
        t0 = time.perf_counter()
        fit()
        out.append(time.perf_counter() - t0)
    rec["fit_transform_s"] = median(out)
    return rec


def time_sklearn(n, d, centres):
    from sklearn.manifold import TSNE
    X = data(n, d, centres)
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        TSNE(n_components=2, random_state=42).fit_transform(X)
        out.append(time.perf_counter() - t0)
    return median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "tsne_timing.json"))
    ap.add_argument("--shapes", default="all", choices=("small", "large", "all"))
    ap.add_argument("--sklearn", action="store_true", help="also time sklearn's TSNE on the host (small shapes)")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    shapes = (SMALL if args.shapes != "large" else []) + (LARGE if args.shapes != "small" else [])
    result = {"threads": int(os.environ.get("OMP_NUM_THREADS", "0")), "shapes": []}
    if os.path.exists(args.out):              # the shapes of an earlier call are kept
        with open(args.out) as f:
            result = json.load(f)
    for n, d, centres in shapes:
        rec = time_shape(n, d, centres, dev)
        if args.sklearn and n <= 20000:
            rec["sklearn_fit_transform_s"] = time_sklearn(n, d, centres)
        result["shapes"] = [r for r in result["shapes"] if (r["n"], r["d"]) != (n, d)] + [rec]
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
