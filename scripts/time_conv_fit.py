"""Time the reference's Hybrid VAE fit (src/Convolutional_VAE.py:202-271) at its own size -- 1336 x 1 x 128 x 1024 mel
(synthetic, generated on the device, about 700 MB) plus 768-d text, batch 32, 85 / 15 split, a fixed 5 epochs with early
stopping disabled = 5 x (36 training steps + 7 validation batches) -- on one MI355X:

  fit      hlmc_amd.fit_conv_vae: per step one hlmc_batch_gather per input and the Trainer.step chain; the validation
           pass through the engine's eval forward and hlmc_loss_sums into a device table; one read-back per epoch
  user     the loop a user of the package wrote around Trainer.step before fit_conv_vae existed: a host-side row gather
           (index slice uploaded, X[idx] per input), Trainer.step and loss_tuple (one read-back and synchronise) per
           step, the validation pass through the module path (model(audio, text), loss_function, .item() per batch)

Every leg runs in a child process of its own under ``timeout -k 10 <--leg-timeout>`` (a hung leg is killed from outside;
nothing else is started after a leg that failed): the child generates the data, runs the leg once untimed as its
warm-up and once timed -- a whole fit, model construction excluded, timed by the host clock to its final read-back --
and prints one JSON line.  After one untimed warm-up round of both legs, --rounds rounds alternate the legs.  Writes one
JSON document (--out) and prints it.

    python scripts/time_conv_fit.py --out profiles/r19/conv_fit_timing.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hlmc_amd  # noqa: E402

# What differs per step between the two loops, counted from the code (train.py); the forward / loss / backward / Adam
# chain of Trainer.step is the same in both.
COUNTS = {
    "user": {
        "rows of a training batch": "1 index slice uploaded (host-to-device copy) + 1 index kernel per input tensor (2)",
        "training loss": "loss_tuple: 1 device-to-host copy of 3 doubles and a synchronise per step",
        "rows of a validation batch": "1 index slice uploaded + 1 index kernel per input tensor (2)",
        "validation batch": "module forward (autograd Function, outputs and workspace allocated per call) + "
                            "loss_function (hlmc_loss_sums + torch arithmetic on the sums) + .item(): 1 read-back and "
                            "synchronise per batch",
    },
    "fit": {
        "rows of a training batch": "1 hlmc_batch_gather launch per input tensor (2) from the resident data and order",
        "training loss": "sums written to the step's row of the epoch's device table",
        "rows of a validation batch": "1 hlmc_batch_gather launch per input tensor (2)",
        "validation batch": "hlmc_net_forward(train=0) into preallocated outputs + hlmc_loss_sums into the table",
        "epoch end": "1 hlmc_fit_epoch_totals launch + 1 read-back of 5 doubles: the epoch's only synchronisation",
    },
}


def build(a):
    torch.manual_seed(42)
    m = hlmc_amd.HybridVAE(128, 768, (a.h, a.w)).cuda()
    torch.manual_seed(7)
    torch.cuda.synchronize()
    return m


def leg_fit(audio, text, split, a):
    m = build(a)
    t0 = time.perf_counter()
    res = hlmc_amd.fit_conv_vae(m, audio, text, epochs=a.epochs, batch_size=a.batch, patience=10 ** 9, split=split)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res.history["val_loss"]


def leg_user(audio, text, split, a):
    m = build(a)
    t0 = time.perf_counter()
    train_idx, val_idx = split
    bs, nt, nv = a.batch, len(train_idx), len(val_idx)
    tr = hlmc_amd.Trainer(m, lr=1e-4)
    hist = []
    for _ in range(a.epochs):
        m.train()
        order = train_idx[hlmc_amd.dataloader_order(nt)]
        ep = 0.0
        for k in range((nt + bs - 1) // bs):
            idx = order[k * bs:(k + 1) * bs].cuda()
            ep += tr.loss_tuple(tr.step(audio[idx], text[idx]))[0]
        m.eval()
        val = 0.0
        with torch.no_grad():
            for j in range((nv + bs - 1) // bs):
                idx = val_idx[j * bs:(j + 1) * bs].cuda()
                x, y = audio[idx], text[idx]
                ra, rt, mu, lv = m(x, y)
                val += hlmc_amd.loss_function(ra, x, rt, y, mu, lv)[0].item()
        hist.append(val / nv)
    tr.release()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, np.asarray(hist)


def summary(ts, steps):
    ts = sorted(ts)
    return {"seconds": [round(t, 4) for t in ts], "median_s": round(float(np.median(ts)), 4), "min_s": round(ts[0], 4),
            "max_s": round(ts[-1], 4), "spread_s": round(ts[-1] - ts[0], 4),
            "median_us_per_step": round(1e6 * float(np.median(ts)) / steps, 1)}


LEGS = {"fit": leg_fit, "user": leg_user}


def run_leg(a):
    """The child: data, one untimed run of the leg, one timed; one JSON line."""
    g = torch.Generator(device="cuda").manual_seed(0)
    audio = torch.randn(a.n, 1, a.h, a.w, device="cuda", generator=g)
    text = torch.randn(a.n, 768, device="cuda", generator=g) / 768 ** 0.5
    train = int(0.85 * a.n)
    split = hlmc_amd.random_split_indices(a.n, [train, a.n - train], torch.Generator().manual_seed(1))
    LEGS[a.leg](audio, text, split, a)
    t, h = LEGS[a.leg](audio, text, split, a)
    print(json.dumps({"leg": a.leg, "seconds": t, "last_epoch_val_loss": float(h[-1])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1336)
    ap.add_argument("--h", type=int, default=128)
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=150)
    ap.add_argument("--leg", choices=sorted(LEGS), help="run this one leg in this process (what the children do)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "conv_fit_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_conv_fit.py measures on the GPU: none is visible")
    if a.leg:
        return run_leg(a)
    train = int(0.85 * a.n)
    nb = (train + a.batch - 1) // a.batch
    nvb = (a.n - train + a.batch - 1) // a.batch
    steps = a.epochs * nb
    times = {k: [] for k in LEGS}
    last = {}
    child = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--n", str(a.n),
             "--h", str(a.h), "--w", str(a.w), "--epochs", str(a.epochs), "--batch", str(a.batch)]
    for r in range(a.rounds + 1):   # round 0 warms the machine up and is not timed
        for k in LEGS:
            p = subprocess.run(child + ["--leg", k], stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:   # a failed or killed leg ends the measurement: nothing more is started
                sys.exit(f"leg {k} of round {r} ended with status {p.returncode}")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            last[k] = rec["last_epoch_val_loss"]
            if r:
                times[k].append(rec["seconds"])
            print(f"round {r} {k}: {rec['seconds']:.3f} s, last epoch val loss {last[k]:.6f}", flush=True)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "fit": {"n": a.n, "input_hw": [a.h, a.w], "text_dim": 768, "latent": 128, "epochs": a.epochs, "batch": a.batch,
                   "training_rows": train, "validation_rows": a.n - train, "training_steps_per_epoch": nb,
                   "validation_batches_per_epoch": nvb, "training_steps": steps,
                   "early_stopping": "disabled (patience 10**9)"},
           "rounds": a.rounds, "legs": {k: summary(v, steps) for k, v in times.items()},
           "what_differs_per_step_from_the_code": COUNTS, "last_epoch_val_loss": last}
    f, u = res["legs"]["fit"], res["legs"]["user"]
    res["fit_ahead_of_user_by_more_than_the_spread"] = bool(u["min_s"] - f["max_s"] > max(f["spread_s"], u["spread_s"]))
    res["ratio_of_medians_user_over_fit"] = round(u["median_s"] / f["median_s"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
