"""Time the batched silhouette against one silhouette_score call per labelling (DESIGN.md "Batched silhouette").

    python scripts/time_silhouette_batch.py --out new.json [--tree DIR] [--parent parent.json] [--steps ...]

One process, a host clock around each synchronised call, one warm-up, medians.  Steps:

  scores100k, scores1336   ks = 2..14 on blob labels at 100,000 x 128 and 1,336 x 128 (the reference's own size):
                           (a) 13 metrics.silhouette_score calls, (b) one metrics.silhouette_scores call (where the
                           tree has it), and whether the two give the same bits
  dbscan100k               dbscan_eps_sweep, the reference's 17 radii at 100,000 x 128
  ward20k                  agglomerative_k_sweep, k = 2..14 at 20,000 x 128

``--tree DIR`` imports the package from another checkout (the parent commit, built) instead of this one: run the script
once per tree on the same machine in the same session, then pass the parent's file with ``--parent`` to the run on the
new tree; its output then carries both sets of numbers and the ratios parent / new.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128
KS = list(range(2, 15))
SWEEP = [float(e) for e in range(3, 20)]


def blobs(n, d=D, k=14, seed=0, spread=3.0):
    """k Gaussian blobs (std 1) around N(0, spread^2) centres, float32, and the blob of each row."""
    import numpy as np
    rng = np.random.default_rng(seed)
    c = rng.normal(0, spread, (k, d))
    y = rng.integers(0, k, n)
    y[rng.permutation(n)[:k]] = np.arange(k)
    return (c[y] + rng.normal(0, 1.0, (n, d))).astype(np.float32), y


def median(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def step_scores(hlmc_amd, n, reps):
    import numpy as np
    import torch
    M = hlmc_amd.metrics
    X, y = blobs(n)
    Xd = torch.from_numpy(X).cuda()
    labelings = [(y % k).astype(np.int64) for k in KS]          # blob labels folded to k = 2..14: every label occurs
    out = {"n": n, "d": D, "ks": [KS[0], KS[-1]], "reps": reps}
    res = {}
    out["per_call_s"] = median(lambda: res.update(a=[M.silhouette_score(Xd, lab) for lab in labelings]), reps)
    if hasattr(M, "silhouette_scores"):
        out["batched_s"] = median(lambda: res.update(b=M.silhouette_scores(Xd, labelings)), reps)
        out["same_bits"] = bool(np.array(res["a"], dtype=np.float64).tobytes() == res["b"].tobytes())
    out["scores"] = [float(s) for s in res["a"]]
    return out


def step_dbscan(hlmc_amd, reps):
    import numpy as np
    import torch
    X, _ = blobs(100000, k=10)
    Xd = torch.from_numpy(X).cuda()
    res = {}
    t = median(lambda: res.update(r=hlmc_amd.dbscan_eps_sweep(Xd, np.array(SWEEP))), reps)
    recs = res["r"][1]
    return {"n": 100000, "d": D, "radii": len(SWEEP), "reps": reps, "sweep_s": t, "best_eps": res["r"][0],
            "scored": sum(r["silhouette"] is not None for r in recs), "clusters": [r["n_clusters"] for r in recs],
            "silhouettes": [r["silhouette"] for r in recs]}


def step_ward(hlmc_amd, reps):
    import torch
    X, _ = blobs(20000, k=10)
    Xd = torch.from_numpy(X).cuda()
    res = {}
    t = median(lambda: res.update(r=hlmc_amd.agglomerative_k_sweep(Xd)), reps)
    return {"n": 20000, "d": D, "ks": [KS[0], KS[-1]], "reps": reps, "sweep_s": t, "best_k": res["r"][0],
            "silhouettes": [r["silhouette"] for r in res["r"][1]]}


STEPS = {"scores100k": lambda h: step_scores(h, 100000, 5), "scores1336": lambda h: step_scores(h, 1336, 21),
         "dbscan100k": lambda h: step_dbscan(h, 3), "ward20k": lambda h: step_ward(h, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=ROOT, help="checkout to import hlmc_amd from (default: this one)")
    ap.add_argument("--parent", default=None, help="results of a run with --tree <parent checkout>, to compare against")
    ap.add_argument("--steps", default=",".join(STEPS))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import hlmc_amd
    results = {"tree": "parent" if args.parent is None and os.path.abspath(args.tree) != ROOT else "new"}
    for name in args.steps.split(","):
        results[name] = STEPS[name](hlmc_amd)
        print(name, json.dumps(results[name]), flush=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    if args.parent:
        parent = json.load(open(args.parent))
        cmp = {}
        for name in args.steps.split(","):
            if name not in parent:
                continue
            p, q = parent[name], results[name]
            if name.startswith("scores"):
                cmp[name] = {"a_parent_13_calls_s": p["per_call_s"], "b_new_one_call_s": q["batched_s"],
                             "ratio_a_over_b": p["per_call_s"] / q["batched_s"],
                             "same_scores_as_parent": p["scores"] == q["scores"] and q["same_bits"]}
            else:
                cmp[name] = {"parent_s": p["sweep_s"], "new_s": q["sweep_s"], "ratio_parent_over_new": p["sweep_s"] / q["sweep_s"],
                             "same_silhouettes_as_parent": p["silhouettes"] == q["silhouettes"]}
        results = {"new": results, "parent": parent, "comparison": cmp}
        print("comparison", json.dumps(cmp, indent=1), flush=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
