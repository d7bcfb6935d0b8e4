"""Time the reference's Simple VAE fit (src/Simple_VAE.py:131-226) at its own size -- 1336 x 370 features, hidden
[128, 64, 32], latent 32, batch 32, 50 epochs with early stopping disabled = 2100 Adam steps -- on one MI355X:

  fit      hlmc_amd.fit_vae: per step one gather launch, one mask launch and the Trainer.step chain; one read-back per
           epoch
  user     the loop a user of the package wrote around Trainer.step before fit_vae existed: a host-side row gather,
           Trainer.step(x) with eps=None (the engine's stream) and dropout=None (VAE.make_dropout_mask: three torch
           launches, then the engine's copy of the mask), loss_tuple (one read-back and synchronise) per step, a live
           ReduceLROnPlateau, the reference's counter, deepcopy(state_dict()) at improvements
  hand     tests/fit_cases.py hand_loop, the bit-for-bit comparison loop of the tests.  NOT a user's loop: every step it
           also restates the dropout mask on the host (a ten-round Philox in numpy, a few hundred microseconds at this
           shape) and uploads it and hlmc_randn's eps synchronously, so that its bits equal fit_vae's.  Timed only to
           show what that costs
  torch    the oracle module (oracle/models_oracle.VAE) in eager torch on the same GPU: X resident, the reference's
           loop as written (nn.Dropout, randn_like, torch.optim.Adam, ReduceLROnPlateau, three .item() per step)

The legs alternate inside each of --rounds rounds after one untimed warm-up round; every leg is a whole fit (model
construction excluded) timed by the host clock to its final read-back.  Writes one JSON document (--out) and prints it.

    python scripts/time_vae_fit.py --out profiles/r18/vae_fit_timing.json
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hlmc_amd  # noqa: E402
from oracle import models_oracle as OM  # noqa: E402
from tests import fit_cases as FC  # noqa: E402

# What differs per train step between the two loops of this package, counted from the code (train.py, models.py,
# csrc/engine.cpp SimpleNet::stage_dropout); the forward / loss / backward / Adam chain of Trainer.step is the same in both.
COUNTS = {
    "user (Trainer.step as a user had to call it)": {
        "row gather": "order[k*bs:(k+1)*bs].to(device) (a host-to-device copy) + X[idx] (one index kernel)",
        "dropout mask": "VAE.make_dropout_mask: 3 torch launches (rand, >=, cast to uint8)",
        "mask staging": "1 device-to-device copy into the workspace (SimpleNet::stage_dropout)",
        "eps": "drawn by the engine (0 extra launches)",
        "loss": "loss_tuple: 1 device-to-host copy of 3 doubles and a synchronise per step",
    },
    "fit (fit_vae)": {
        "row gather": "1 hlmc_batch_gather launch from the resident X and the epoch's resident order",
        "dropout mask": "1 hlmc_dropout_mask launch straight into the workspace",
        "mask staging": "none",
        "eps": "drawn by the engine (0 extra launches)",
        "loss": "sums written to the step's row of the epoch table; per EPOCH 1 hlmc_vae_epoch_means launch and 1 "
                "read-back of 3 doubles",
    },
    "hand (tests/fit_cases.py hand_loop) on top of user": "per step a host numpy Philox restatement of the mask, its "
                                                          "synchronous upload, 1 hlmc_randn launch for eps",
}


def make_data(n, d):
    g = torch.Generator().manual_seed(0)
    return torch.randn(n, d, generator=g)


def build(a, cls):
    torch.manual_seed(42)
    m = cls(a.d, list(a.hidden), a.latent).cuda()
    torch.manual_seed(7)
    torch.cuda.synchronize()
    return m


def leg_fit(Xd, a):
    m = build(a, hlmc_amd.VAE)
    t0 = time.perf_counter()
    res = hlmc_amd.fit_vae(m, Xd, epochs=a.epochs, batch_size=a.batch, patience=10 ** 9)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res.history["loss"]


def leg_hand(Xd, a):
    m = build(a, hlmc_amd.VAE)
    t0 = time.perf_counter()
    res = FC.hand_loop(m, Xd, epochs=a.epochs, batch_size=a.batch, patience=10 ** 9)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res["history"]["loss"]


def leg_user(Xd, a):
    m = build(a, hlmc_amd.VAE)
    t0 = time.perf_counter()
    n, bs = Xd.shape[0], a.batch
    nb = (n + bs - 1) // bs
    m.train()
    tr = hlmc_amd.Trainer(m, lr=1e-4, beta=0.8)
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(dummy, mode="min", factor=0.5, patience=15)
    hist, best, state = [], float("inf"), None
    for _ in range(a.epochs):
        order = hlmc_amd.dataloader_order(n)
        ep = 0.0
        for k in range(nb):
            xb = Xd[order[k * bs:(k + 1) * bs].cuda()]
            ep += tr.loss_tuple(tr.step(xb), batch=xb.shape[0])[0]
        avg = ep / nb
        hist.append(avg)
        sched.step(avg)
        tr.lr = float(dummy.param_groups[0]["lr"])
        if avg < best:
            best, state = avg, copy.deepcopy(m.state_dict())
    tr.release()
    m.load_state_dict(state)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, np.asarray(hist)


def leg_torch(Xd, a):
    m = build(a, OM.VAE)
    t0 = time.perf_counter()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=15)
    n = Xd.shape[0]
    nb = (n + a.batch - 1) // a.batch
    hist, best = [], float("inf")
    for _ in range(a.epochs):
        m.train()
        order = hlmc_amd.dataloader_order(n).cuda()
        ep = [0.0, 0.0, 0.0]
        for k in range(nb):
            x = Xd[order[k * a.batch:(k + 1) * a.batch]]
            recon, mu, logvar, _ = m(x)
            loss, rl, kl = OM.vae_loss(recon, x, mu, logvar, 0.8)
            opt.zero_grad()
            loss.backward()
            opt.step()
            ep[0] += loss.item()
            ep[1] += rl.item()
            ep[2] += kl.item()
        avg = ep[0] / nb
        hist.append(avg)
        sched.step(avg)
        if avg < best:
            best = avg
            state = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_state_dict(state)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, np.asarray(hist)


def summary(ts, steps):
    ts = sorted(ts)
    return {"seconds": [round(t, 4) for t in ts], "median_s": round(float(np.median(ts)), 4), "min_s": round(ts[0], 4),
            "max_s": round(ts[-1], 4), "spread_s": round(ts[-1] - ts[0], 4),
            "median_us_per_step": round(1e6 * float(np.median(ts)) / steps, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1336)
    ap.add_argument("--d", type=int, default=370)
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 64, 32])
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "vae_fit_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_vae_fit.py measures on the GPU: none is visible")
    Xd = make_data(a.n, a.d).cuda()
    steps = a.epochs * ((a.n + a.batch - 1) // a.batch)
    legs = {"fit": lambda: leg_fit(Xd, a), "user": lambda: leg_user(Xd, a), "hand": lambda: leg_hand(Xd, a),
            "torch": lambda: leg_torch(Xd, a)}
    times = {k: [] for k in legs}
    hists = {}
    for r in range(a.rounds + 1):   # round 0 warms every leg up and is not timed
        for k, f in legs.items():
            t, h = f()
            hists[k] = h
            if r:
                times[k].append(t)
            print(f"round {r} {k}: {t:.3f} s, last epoch loss {h[-1]:.6f}", flush=True)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "fit": {"n": a.n, "d": a.d, "hidden": list(a.hidden), "latent": a.latent, "epochs": a.epochs, "batch": a.batch,
                   "steps": steps, "early_stopping": "disabled (patience 10**9)"},
           "rounds": a.rounds, "legs": {k: summary(v, steps) for k, v in times.items()},
           "what_differs_per_step_from_the_code": COUNTS,
           "same_results": {"fit_equals_hand_bit_for_bit": bool(np.array_equal(hists["fit"], hists["hand"])),
                            "last_epoch_loss": {k: float(h[-1]) for k, h in hists.items()}}}
    f, u, h, t = (res["legs"][k] for k in ("fit", "user", "hand", "torch"))
    res["fit_ahead_of_user_by_more_than_the_spread"] = bool(u["min_s"] - f["max_s"] > max(f["spread_s"], u["spread_s"]))
    res["ratio_of_medians"] = {"user_over_fit": round(u["median_s"] / f["median_s"], 2),
                               "torch_gpu_over_fit": round(t["median_s"] / f["median_s"], 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
