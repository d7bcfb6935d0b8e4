"""Time the reference's autoencoder baseline fit (src/Conditional_VAE.py:428-452) at its own size -- 1336 x 290
features, latent 64, 50 epochs at batch 32 = 2100 Adam steps -- on one MI355X:

  graph    hlmc_amd.fit_autoencoder(graph=True):  per step one gather launch, one coefficient copy, one graph replay
  eager    hlmc_amd.fit_autoencoder(graph=False): the same kernels launched one by one
  torch    the oracle module (oracle/models_oracle.SimpleAutoencoder) in eager torch on the same GPU: X resident, the
           same row order, mse_loss, torch.optim.Adam, the epoch loss accumulated on the device (no per-batch .item())
  cpu      the oracle loop with a DataLoader on the host's threads (once; --cpu-threads)

The three GPU legs alternate inside each of --rounds rounds after one untimed warm-up round; every leg is a whole fit
(model construction excluded, trainer construction, capture and the final read-back included) timed by the host clock
around work that ends in a device synchronise.  Writes one JSON document (--out) and prints it.

    python scripts/time_autoencoder.py --out profiles/r17/ae_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hlmc_amd  # noqa: E402
from oracle import models_oracle as OM  # noqa: E402

# Stream operations per train step, counted from the code (csrc/engine.cpp AeNet, csrc/autoencoder.hip, train.py):
#   forward   1 cast of x + 6 GEMMs (bias and ReLU in the epilogue)
#   loss      1 (hlmc_mse_rows at 32 x 290: the one-block form)
#   backward  1 cast of d_recon + 5 data-gradient GEMMs (ReLU mask in the epilogue) + 6 weight+bias-gradient GEMMs
#   Adam      1 (every parameter and the repacked GEMM weights)
# = 21 kernels, plus a split-K reduce launch behind any GEMM the tile plan splits, plus 3 forks and 1 join of the
# weight-gradient stream (an event record and a stream wait each).
COUNTS = {
    "kernels_in_step": 21,
    "eager": {"host_launch_calls_per_step": 21 + 1 + 1, "what": "21 step kernels + hlmc_batch_gather + coefficient copy",
              "event_record_wait_pairs_per_step": 4, "c_abi_calls_per_step": 6},
    "graph": {"host_launch_calls_per_step": 3, "what": "hlmc_batch_gather + coefficient copy + hipGraphLaunch",
              "event_record_wait_pairs_per_step": 0, "c_abi_calls_per_step": 2},
}


def make_data(n, d):
    g = torch.Generator().manual_seed(0)
    return torch.randn(n, d, generator=g)


def leg_ours(Xd, a, graph):
    torch.manual_seed(42)
    m = hlmc_amd.SimpleAutoencoder(a.d, a.latent).cuda()
    torch.manual_seed(7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = hlmc_amd.fit_autoencoder(m, Xd, epochs=a.epochs, batch_size=a.batch, graph=graph)
    return time.perf_counter() - t0, hist


def leg_torch(Xd, a):
    torch.manual_seed(42)
    m = OM.SimpleAutoencoder(a.d, a.latent).cuda()
    torch.manual_seed(7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    n = Xd.shape[0]
    nb = (n + a.batch - 1) // a.batch
    hist = torch.zeros(a.epochs, dtype=torch.float64, device="cuda")
    for e in range(a.epochs):
        order = hlmc_amd.dataloader_order(n).cuda()
        tot = torch.zeros((), device="cuda")
        for k in range(nb):
            xb = Xd[order[k * a.batch:(k + 1) * a.batch]]
            opt.zero_grad()
            loss = F.mse_loss(m(xb)[0], xb)
            loss.backward()
            opt.step()
            tot += loss.detach()
        hist[e] = tot / nb
    out = hist.cpu().numpy()
    return time.perf_counter() - t0, out


def leg_cpu(X, a):
    torch.set_num_threads(a.cpu_threads)
    torch.manual_seed(42)
    m = OM.SimpleAutoencoder(a.d, a.latent)
    torch.manual_seed(7)
    t0 = time.perf_counter()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    loader = DataLoader(TensorDataset(X), batch_size=a.batch, shuffle=True)
    hist = []
    for _ in range(a.epochs):
        tot = 0.0
        for (xb,) in loader:
            opt.zero_grad()
            loss = F.mse_loss(m(xb)[0], xb)
            loss.backward()
            opt.step()
            tot += loss.item()
        hist.append(tot / len(loader))
    return time.perf_counter() - t0, np.array(hist)


def summary(ts, steps):
    ts = sorted(ts)
    return {"seconds": [round(t, 4) for t in ts], "median_s": round(float(np.median(ts)), 4), "min_s": round(ts[0], 4),
            "max_s": round(ts[-1], 4), "spread_s": round(ts[-1] - ts[0], 4),
            "median_us_per_step": round(1e6 * float(np.median(ts)) / steps, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1336)
    ap.add_argument("--d", type=int, default=290)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "ae_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_autoencoder.py measures on the GPU: none is visible")
    X = make_data(a.n, a.d)
    Xd = X.cuda()
    steps = a.epochs * ((a.n + a.batch - 1) // a.batch)
    legs = {"graph": lambda: leg_ours(Xd, a, True), "eager": lambda: leg_ours(Xd, a, False), "torch": lambda: leg_torch(Xd, a)}
    times = {k: [] for k in legs}
    hists = {}
    for r in range(a.rounds + 1):   # round 0 warms every leg up and is not timed
        for k, f in legs.items():
            t, h = f()
            hists[k] = h
            if r:
                times[k].append(t)
            print(f"round {r} {k}: {t:.3f} s, last epoch loss {h[-1]:.6f}", flush=True)
    t_cpu, h_cpu = leg_cpu(X, a)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "fit": {"n": a.n, "d": a.d, "latent": a.latent, "epochs": a.epochs, "batch": a.batch, "steps": steps},
           "rounds": a.rounds, "legs": {k: summary(v, steps) for k, v in times.items()},
           "cpu_oracle_loop": {"threads": a.cpu_threads, "seconds": round(t_cpu, 3),
                               "us_per_step": round(1e6 * t_cpu / steps, 1)},
           "per_step_counts_from_the_code": COUNTS,
           "same_results": {"graph_equals_eager_bit_for_bit": bool(np.array_equal(hists["graph"], hists["eager"])),
                            "max_rel_loss_diff_vs_torch_gpu": float(np.max(np.abs(hists["graph"] - hists["torch"]) /
                                                                            np.abs(hists["torch"]))),
                            "max_rel_loss_diff_vs_cpu_oracle": float(np.max(np.abs(hists["graph"] - h_cpu) / np.abs(h_cpu)))}}
    g, e = res["legs"]["graph"], res["legs"]["eager"]
    res["graph_beats_eager_by_more_than_the_spread"] = bool(e["min_s"] - g["max_s"] > max(g["spread_s"], e["spread_s"]))
    res["speedup_median"] = {"graph_vs_eager": round(e["median_s"] / g["median_s"], 2),
                             "graph_vs_torch_gpu": round(res["legs"]["torch"]["median_s"] / g["median_s"], 2),
                             "graph_vs_cpu_oracle": round(t_cpu / g["median_s"], 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
