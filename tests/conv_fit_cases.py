"""Shared helpers of the fit_conv_vae tests (tests/test_conv_fit_cpu.py, tests/test_conv_fit_gpu.py): the host
restatement of hlmc_fit_epoch_totals, small data sets, and the two convolutional
scripts' loops (src/Convolutional_VAE.py:217-271, src/Conditional_VAE.py:310-362) written with what the package offered
before fit_conv_vae existed.

  epoch_totals   hlmc_fit_epoch_totals: Python floats (IEEE float64, one rounding per operation), rows in step order
  make_data      audio / text / one-hot cond of a small data set
  build          the three model kinds of the tests, seeded
  hand_loop      Trainer.step(eps=None) per batch on host-gathered rows with loss_tuple per step, an eval forward plus
                 hlmc_loss_sums with a read-back per validation batch, the sums added on the host, the reference's
                 counter, deepcopy(state_dict()) at improvements
"""
import copy

import numpy as np
import torch


def round4(n):
    return (int(n) + 3) & ~3


def epoch_totals(train_sums, val_sums, text_weight, beta, train_div, val_div):
    """train_sums [nt][3], val_sums [nv][3] -> (train total, audio, text, kld, val total) as hlmc_fit_epoch_totals
    computes them: kld = -0.5 s2, total = (s0 + text_weight s1) + beta kld, added in row order, then divided."""
    tw, beta = float(text_weight), float(beta)
    total = audio = text = kld = val = 0.0
    for s0, s1, s2 in train_sums:
        q = -0.5 * float(s2)
        total += (float(s0) + tw * float(s1)) + beta * q
        audio += float(s0)
        text += float(s1)
        kld += q
    for s0, s1, s2 in val_sums:
        q = -0.5 * float(s2)
        val += (float(s0) + tw * float(s1)) + beta * q
    return total / float(train_div), audio / float(train_div), text / float(train_div), kld / float(train_div), \
        val / float(val_div)


def epoch_totals_cases(nt, nv, seed=0):
    """Loss-sum tables whose values span 1e-3 .. 1e9 in magnitude, s[2] of both signs."""
    rng = np.random.default_rng(1000 * nt + nv + seed)

    def table(rows):
        mag = 10.0 ** rng.uniform(-3, 9, (rows, 3))
        sign = np.where(rng.random((rows, 3)) < 0.5, -1.0, 1.0)
        sign[:, :2] = 1.0                       # squared errors are non-negative; s[2] takes both signs
        t = mag * sign
        t[0, 2] = -abs(t[0, 2])                 # at least one negative s[2] (the usual sign) ...
        if rows > 1:
            t[1, 2] = abs(t[1, 2])              # ... and one positive
        return t
    return table(nt), table(nv)


# ---------------------------------------------------------------------------------------------------- models and data
KINDS = {"hybrid": dict(hw=(64, 64), text_dim=768, latent=128),
         "audio": dict(hw=(64, 128), text_dim=0, latent=64),
         "cvae": dict(hw=(64, 64), text_dim=384, latent=64, classes=10)}


def build(kind, seed, device="cuda"):
    import hlmc_amd
    c = KINDS[kind]
    torch.manual_seed(seed)
    if kind == "cvae":
        m = hlmc_amd.ConditionalVAE(c["latent"], c["text_dim"], c["classes"], c["hw"])
    else:
        m = hlmc_amd.HybridVAE(c["latent"], c["text_dim"] or 768, c["hw"], audio_only=kind == "audio")
    return m.to(device) if device else m


def make_data(kind, n, seed=3):
    """(audio [n][1][H][W], text [n][text_dim] or None, cond one-hot [n][classes] or None), CPU float32."""
    c = KINDS[kind]
    g = torch.Generator().manual_seed(seed)
    H, W = c["hw"]
    audio = torch.randn(n, 1, H, W, generator=g) + 0.5 * torch.randn(n, 1, 1, 1, generator=g)
    text = torch.randn(n, c["text_dim"], generator=g) / c["text_dim"] ** 0.5 if c["text_dim"] else None
    cond = None
    if kind == "cvae":
        cond = torch.zeros(n, c["classes"])
        cond[torch.arange(n), torch.arange(n) % c["classes"]] = 1.0
    return audio, text, cond


def batch_sizes(rows, bs):
    return [bs] * (rows // bs) + ([rows % bs] if rows % bs else [])


# ---------------------------------------------------------------------------------------------------- the hand loop
def eval_sums(model, a, t, c):
    """Loss sums (host list of 3 doubles) of an eval-mode engine forward on one batch, eps from the net's stream."""
    from hlmc_amd import _lib as L
    lib, net, dev, B = L.lib(), model._native_net(), a.device, a.shape[0]
    out = model._alloc_outputs(B, dev)
    ws = net.new_workspace(B, dev)
    L.check(lib.hlmc_net_forward(net.h, L.stream(), B, 0, L.ptr(a), L.ptr(t), L.ptr(c), None, None, L.ptr(out["recon"]),
                                 L.ptr(out.get("recon_text")), L.ptr(out["mu"]), L.ptr(out["logvar"]), None,
                                 ws.data_ptr()), "hlmc_net_forward")
    na, nl = out["recon"].numel(), out["mu"].numel()
    nt = out["recon_text"].numel() if "recon_text" in out else 0
    lws = torch.empty(max(16, int(lib.hlmc_loss_workspace(na, nt, nl))), dtype=torch.uint8, device=dev)
    sums = torch.zeros(3, dtype=torch.float64, device=dev)
    L.check(lib.hlmc_loss_sums(L.stream(), L.ptr(out["recon"]), L.ptr(a), na, L.ptr(out.get("recon_text")),
                               L.ptr(t if nt else None), nt, L.ptr(out["mu"]), L.ptr(out["logvar"]), nl, sums.data_ptr(),
                               lws.data_ptr()), "hlmc_loss_sums")
    s = sums.cpu().tolist()
    L.check_device("eval_sums")
    return s


def hand_loop(model, audio, text, cond, train_idx, val_idx, *, epochs, batch_size, lr=1e-4, beta, text_weight, patience,
              normalize, generator=None, restore_best=False):
    """The reference loop with the package's older pieces.  audio / text / cond: float32 device tensors (None where the
    model takes none); train_idx / val_idx: int64 CPU tensors.  Returns a dict with fit_conv_vae's fields plus
    ``pre_val_state``: a deep copy of the state_dict taken after the last training step of the last epoch run, before
    its validation pass."""
    import hlmc_amd
    from hlmc_amd.train import dataloader_order

    dev, bs = audio.device, int(batch_size)
    nt_rows, nv_rows = len(train_idx), len(val_idx)
    tr = hlmc_amd.Trainer(model, lr=lr, beta=beta, text_weight=text_weight)
    ntb, nvb = len(batch_sizes(nt_rows, bs)), len(batch_sizes(nv_rows, bs))
    divs = (nt_rows, nv_rows) if normalize == "samples" else (ntb, nvb)
    keys = ("train_loss", "audio", "text", "kld", "val_loss")
    hist = {k: [] for k in keys}
    best_loss, counter, best_epoch, best_state, stopped, pre_val = float("inf"), 0, None, None, None, None

    def rows(idx):
        idx = idx.to(dev)                                  # the host-side row gather
        return [None if x is None else x[idx] for x in (audio, text, cond)]

    for e in range(epochs):
        model.train()
        order = train_idx[dataloader_order(nt_rows, generator)]
        ep = [0.0, 0.0, 0.0, 0.0]
        for k in range(ntb):
            a, t, c = rows(order[k * bs:(k + 1) * bs])
            tup = tr.loss_tuple(tr.step(a, t, c, eps=None))
            for i in range(4):
                ep[i] += tup[i]
        pre_val = copy.deepcopy(model.state_dict())
        model.eval()
        val = 0.0
        for j in range(nvb):
            a, t, c = rows(val_idx[j * bs:(j + 1) * bs])
            s = eval_sums(model, a, t, c)
            val += (s[0] + float(text_weight) * s[1]) + float(beta) * (-0.5 * s[2])
        figures = [v / float(divs[0]) for v in ep] + [val / float(divs[1])]
        for key, v in zip(keys, figures):
            hist[key].append(v)
        if figures[4] < best_loss:
            best_loss, counter, best_epoch = figures[4], 0, e
            best_state = copy.deepcopy(model.state_dict())
        else:
            counter += 1
        if counter >= patience:
            stopped = e
            break
    tr.release()
    if restore_best and best_state is not None:
        model.load_state_dict(best_state)
    model.eval()
    return {"history": {k: np.asarray(v, dtype=np.float64) for k, v in hist.items()}, "best_epoch": best_epoch,
            "best_val_loss": best_loss, "stopped_epoch": stopped, "best_state": best_state, "pre_val_state": pre_val,
            "eps_rng": model.get_rng_state()}


# ---------------------------------------------------------------------------------------------------- recorded fits
# labellings and scores as the experiments' row builders receive them (recorded, not computed: the builders are pure)
RECORDED_CONV = {
    "best": (5, 3, 7.0),
    "labels": [np.arange(20) % 5, np.arange(20) % 2, np.arange(20) % 3, np.array([0] * 12 + [-1] * 8)],
    "scores": [{"Silhouette": 0.25, "Davies-Bouldin": 1.5, "ARI": 0.125},
               {"Silhouette": 0.5, "Davies-Bouldin": 0.75, "ARI": 0.0625},
               {"Silhouette": 0.375, "Davies-Bouldin": 1.25, "ARI": None},
               {"Silhouette": 0.875, "Davies-Bouldin": 0.5, "ARI": 0.5}],
}
RECORDED_CVAE = [("CVAE (Multi-Modal)", {"Silhouette": 0.25, "Calinski-Harabasz": 50.0, "NMI": 0.5, "ARI": 0.125,
                                         "Purity": 0.75}),
                 ("PCA + K-Means", {"Silhouette": 0.125, "Calinski-Harabasz": 40.0, "NMI": 0.25, "ARI": 0.0625,
                                    "Purity": 0.5}),
                 ("Autoencoder + K-Means", {"Silhouette": 0.5, "Calinski-Harabasz": 30.0, "NMI": 0.375, "ARI": 0.25,
                                            "Purity": 0.625}),
                 ("Direct Spectral", {"Silhouette": 0.0625, "Calinski-Harabasz": 20.0, "NMI": 0.125, "ARI": 0.03125,
                                      "Purity": 0.375})]
