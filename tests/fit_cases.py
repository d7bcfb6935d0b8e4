"""Shared helpers of the fit_vae tests (tests/test_fit_vae_cpu.py, tests/test_fit_vae_gpu.py) and of
scripts/time_vae_fit.py: host restatements of the two new device ops, and the reference's Simple VAE loop
(src/Simple_VAE.py:131-226) written with what the package offered before fit_vae existed.

  keep_mask_ref     hlmc_dropout_mask, block by block on oracle.rng_oracle.philox4x32 (the definition)
  keep_mask         the same bytes from a vectorised numpy Philox (the hand loop needs ~10^5 blocks); pinned to
                    keep_mask_ref and to the Random123 known-answer blocks by the CPU test
  epoch_means       hlmc_vae_epoch_means: Python floats (IEEE float64, one rounding per operation), step order
  hand_loop         Trainer.step per batch with uploaded eps / masks, loss_tuple per step, a live
                    torch.optim.lr_scheduler.ReduceLROnPlateau, the reference's counter, deepcopy(state_dict()) at
                    improvements
"""
import copy
import math

import numpy as np
import torch

from oracle import rng_oracle as RNG

MASK32 = 0xFFFFFFFF


def threshold(p_drop):
    """T = ceil(p_drop 2^32), the product formed in float64 as on the host side of the library."""
    return int(math.ceil(float(p_drop) * 4294967296.0))


def round4(n):
    return (int(n) + 3) & ~3


def keep_mask_ref(n, p_drop, seed, offset):
    """out[i] = 1 iff word(offset + i) >= T; word g = component g % 4 of Philox4x32-10(counter {g / 4 as 64 bits, 0, 0},
    key {seed low, seed high})."""
    assert offset % 4 == 0
    T = threshold(p_drop)
    out = np.empty(n, np.uint8)
    for t in range((n + 3) // 4):
        q = (offset // 4 + t) & 0xFFFFFFFFFFFFFFFF
        w = RNG.philox4x32((q & MASK32, q >> 32, 0, 0), (seed & MASK32, (seed >> 32) & MASK32))
        for j in range(4):
            if 4 * t + j < n:
                out[4 * t + j] = 1 if w[j] >= T else 0
    return out


def philox_words(seed, q, hi=(0, 0)):
    """Philox4x32-10 blocks at the 64-bit counters q (array) under key `seed`: uint64 array [len(q)][4] of 32-bit words.
    The rounds of RNG.philox4x32 on numpy uint64 lanes (a 32 x 32 bit product fits).  hi: counter words 2 and 3 (zero in
    the library's streams; the known-answer blocks set them)."""
    q = np.asarray(q, dtype=np.uint64)
    m32 = np.uint64(MASK32)
    c0, c1 = q & m32, q >> np.uint64(32)
    c2, c3 = np.full_like(q, hi[0]), np.full_like(q, hi[1])
    k0, k1 = int(seed) & MASK32, (int(seed) >> 32) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(RNG.M0) * c0, np.uint64(RNG.M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + RNG.W0) & MASK32, (k1 + RNG.W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=1)


def keep_mask(n, p_drop, seed, offset):
    assert offset % 4 == 0
    groups = (n + 3) // 4
    q = (np.uint64(offset // 4) + np.arange(groups, dtype=np.uint64))
    words = philox_words(seed, q).reshape(-1)[:n]
    return (words >= np.uint64(threshold(p_drop))).astype(np.uint8)   # 64-bit compare: T reaches 2^32 for p near 1


def epoch_means(sums, na_nl, beta):
    """sums [nb][3], na_nl [nb][2] -> (loss, recon, kl) as hlmc_vae_epoch_means computes them."""
    loss = recon = kl = 0.0
    nb = len(sums)
    for (s0, _, s2), (na, nl) in zip(sums, na_nl):
        r = float(s0) / float(na)
        q = -0.5 * float(s2) / float(nl)
        loss += r + float(beta) * q
        recon += r
        kl += q
    return loss / nb, recon / nb, kl / nb


def hand_loop(model, X, epochs=500, batch_size=32, lr=1e-4, beta=0.8, patience=15, lr_factor=0.5, lr_patience=15,
              generator=None, dropout_seed=None, restore_best=True):
    """The reference loop with the package's older pieces.  X: float32 device tensor [n][d].  The noise is uploaded:
    eps from hlmc_randn and masks from keep_mask, at the offsets the engine's two streams would stand at.  Returns a
    dict with fit_vae's fields."""
    import hlmc_amd
    from hlmc_amd import _lib as L
    from hlmc_amd.train import _DROPOUT_STREAM_KEY, dataloader_order, keyed_seed

    dev, (n, d) = X.device, X.shape
    bs, lat, widths = int(batch_size), model.latent_dim, sum(model.mask_widths())
    model.train()
    tr = hlmc_amd.Trainer(model, lr=lr, beta=beta)
    eps_seed, eps_off = model.get_rng_state()
    drop_seed = keyed_seed(eps_seed, _DROPOUT_STREAM_KEY) if dropout_seed is None else int(dropout_seed)
    drop_off = 0
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(dummy, mode="min", factor=lr_factor, patience=lr_patience)
    hist = {k: [] for k in ("loss", "recon", "kl", "lr")}
    best_loss, counter, best_epoch, best_state, stopped = float("inf"), 0, None, None, None
    nb = (n + bs - 1) // bs
    for e in range(epochs):
        order = dataloader_order(n, generator)
        ep = [0.0, 0.0, 0.0]
        for k in range(nb):
            xb = X[order[k * bs:(k + 1) * bs].to(dev)]   # the host-side row gather
            B = xb.shape[0]
            eps = torch.empty(B, lat, device=dev)
            L.check(L.lib().hlmc_randn(L.stream(), eps.data_ptr(), B * lat, eps_seed, eps_off), "hlmc_randn")
            eps_off += round4(B * lat)
            mask = torch.from_numpy(keep_mask(B * widths, 0.2, drop_seed, drop_off)).to(dev)
            drop_off += round4(B * widths)
            total, recon, _, kl = tr.loss_tuple(tr.step(xb, eps=eps, dropout=mask), batch=B)
            ep[0] += total
            ep[1] += recon
            ep[2] += kl
        avg = [v / nb for v in ep]
        for key, v in zip(("loss", "recon", "kl", "lr"), (*avg, float(tr.lr))):
            hist[key].append(v)
        sched.step(avg[0])
        tr.lr = float(dummy.param_groups[0]["lr"])
        if avg[0] < best_loss:
            best_loss, counter, best_epoch = avg[0], 0, e
            best_state = copy.deepcopy(model.state_dict())
        else:
            counter += 1
        if counter >= patience:
            stopped = e
            break
    tr.release()
    if restore_best and best_state is not None:
        model.load_state_dict(best_state)
    return {"history": {k: np.asarray(v, dtype=np.float64) for k, v in hist.items()}, "best_epoch": best_epoch,
            "best_loss": best_loss, "stopped_epoch": stopped, "best_state": best_state,
            "eps_rng": (eps_seed, eps_off), "dropout_rng": (drop_seed, drop_off)}


# a recorded series: torch halves lr at epoch 53, the run stops at epoch 59, best epoch 44 (0-based)
def slow_descent_series():
    tail = [0.6 * (1.0 - 1e-5) ** i for i in range(1, 41)]
    return [1.0, 0.9, 0.8, 0.7, 0.6] + tail + 30 * [tail[-1]]
