"""fit_vae on the GPU: the device dropout stream (hlmc_dropout_mask, hlmc_net_set_dropout_rng), the epoch means
(hlmc_vae_epoch_means), the whole fit against the hand-written loop it replaces (tests/fit_cases.py hand_loop), the
float64 oracle, and the first script's table (baselines.simple_vae_experiment).

Everything but the oracle comparison is bit for bit: the two loops issue the same arithmetic on the same rows, noise
and masks; only where the noise comes from and when the host looks at the loss differ."""
import ctypes as C

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import models_oracle as OM
from tests import fit_cases as FC

pytestmark = pytest.mark.gpu

# ragged input width, two blocks, sum of mask widths 72.  (The engine's BatchNorm kernels take widths of 4 x a power of
# two, so [24, 12] cannot be built; [32, 4] keeps the 7 x 72 = 504 mask bytes at B = 7.)
SMALL = (37, [32, 4], 5)
REFSHAPE = (370, [128, 64, 32], 32)      # the reference's VAE_CONFIG
GUARD = 64


def _model(cfg, seed):
    torch.manual_seed(seed)
    return hlmc_amd.VAE(cfg[0], list(cfg[1]), cfg[2]).cuda()


def _data(n, d, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) + 2.0 * torch.randn(1, d, generator=g)).cuda()


# ------------------------------------------------------------------------------------------------ the mask op
def test_dropout_mask_bytes_equal_the_restatement(cuda):
    """Every n (empty, below / at / above one Philox block, around one 256-thread block's 1024 bytes), every byte
    alignment of `out`, stream offsets 0 / 4 / 4096 and every p: the bytes of tests/fit_cases.py keep_mask, with the 64
    guard bytes on each side untouched; a second run writes the same bytes."""
    lib, s = L.lib(), L.stream()
    seed = 0x9E3779B97F4A7C15
    for n in (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1025):
        for a in range(4):
            for off in (0, 4, 4096):
                for p in (0.0, 0.2, 0.5):
                    buf = torch.full((GUARD + 4 + n + GUARD,), 0xAB, dtype=torch.uint8, device=cuda)
                    assert buf.data_ptr() % 4 == 0
                    lo = GUARD + a
                    L.check(lib.hlmc_dropout_mask(s, buf.data_ptr() + lo, n, p, seed, off), "hlmc_dropout_mask")
                    got = buf.cpu().numpy()
                    what = f"n={n} align={a} offset={off} p={p}"
                    assert (got[:lo] == 0xAB).all() and (got[lo + n:] == 0xAB).all(), what
                    np.testing.assert_array_equal(got[lo:lo + n], FC.keep_mask(n, p, seed, off), err_msg=what)
                    if p == 0.2 and off == 4:
                        L.check(lib.hlmc_dropout_mask(s, buf.data_ptr() + lo, n, p, seed, off))
                        np.testing.assert_array_equal(buf.cpu().numpy(), got, err_msg=what + " second run")
    assert FC.keep_mask(1025, 0.2, seed, 0).min() == 0 and FC.keep_mask(1025, 0.2, seed, 0).max() == 1


def test_dropout_mask_counter_carries_into_its_high_word(cuda):
    """offset 4 (2^32 - 1), n = 12: the three Philox blocks at counters 2^32 - 1, 2^32, 2^32 + 1."""
    off = 4 * (2 ** 32 - 1)
    for a in (0, 1):
        buf = torch.full((GUARD + 4 + 12 + GUARD,), 0xAB, dtype=torch.uint8, device=cuda)
        L.check(L.lib().hlmc_dropout_mask(L.stream(), buf.data_ptr() + GUARD + a, 12, 0.5, 77, off))
        got = buf.cpu().numpy()
        np.testing.assert_array_equal(got[GUARD + a:GUARD + a + 12], FC.keep_mask_ref(12, 0.5, 77, off))
        assert (got[:GUARD + a] == 0xAB).all() and (got[GUARD + a + 12:] == 0xAB).all()
    # the carry matters: the block at counter 2^32 is not the block at counter 0
    assert not np.array_equal(FC.keep_mask_ref(64, 0.5, 77, 4 * 2 ** 32), FC.keep_mask_ref(64, 0.5, 77, 0))


# ------------------------------------------------------------------------------------------------ the engine's draw
class _Net:
    """hlmc_net_forward / decode / backward on a VAE through the C ABI, with caller-held buffers."""

    def __init__(self, model, B):
        self.m, self.B, self.net = model, B, model._native_net()
        self.dev = next(model.parameters()).device
        self.ws = self.net.new_workspace(B, self.dev)

    def forward(self, x, eps, dropout, train=1):
        out = self.m._alloc_outputs(self.B, self.dev)
        L.check(L.lib().hlmc_net_forward(self.net.h, L.stream(), self.B, train, L.ptr(x), None, None, L.ptr(eps),
                                         L.ptr(dropout), L.ptr(out["recon"]), None, L.ptr(out["mu"]),
                                         L.ptr(out["logvar"]), L.ptr(out["z"]), self.ws.data_ptr()), "hlmc_net_forward")
        return out

    def decode(self, z, dropout, train=1):
        recon = torch.empty(self.B, self.m.input_dim, device=self.dev)
        L.check(L.lib().hlmc_net_decode(self.net.h, L.stream(), self.B, train, L.ptr(z), None, L.ptr(dropout),
                                        L.ptr(recon), None, self.ws.data_ptr()), "hlmc_net_decode")
        return recon

    def backward(self, d):
        L.check(L.lib().hlmc_net_backward(self.net.h, L.stream(), self.B, L.ptr(d["recon"]), None, L.ptr(d["mu"]),
                                          L.ptr(d["logvar"]), self.ws.data_ptr()), "hlmc_net_backward")
        L.check(L.lib().hlmc_net_settle(self.net.h, L.stream()), "hlmc_net_settle")
        return self.m._gflat.clone()


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("recon", "mu", "logvar", "z"))


def test_engine_draws_the_restated_mask(cuda):
    B, seed = 7, 0x1234567887654321
    m = _model(SMALL, 11)
    m.train()
    nmask = B * sum(m.mask_widths())
    assert nmask == 7 * 72 and FC.round4(nmask) == 504
    net = _Net(m, B)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 37, generator=g).cuda()
    eps = torch.randn(B, 5, generator=g).cuda()
    d = {"recon": torch.randn(B, 37, generator=g).cuda(), "mu": torch.randn(B, 5, generator=g).cuda(),
         "logvar": torch.randn(B, 5, generator=g).cuda()}

    def mask(off):
        return torch.from_numpy(FC.keep_mask(nmask, 0.2, seed, off)).cuda()

    assert m.get_dropout_rng_state() == (False, 0, 0)
    plain = net.forward(x, eps, None)                           # today's meaning of NULL: no dropout
    want0 = net.forward(x, eps, mask(0))
    g0 = net.backward(d)
    want1 = net.forward(x, eps, mask(504))
    g1 = net.backward(d)
    assert not _same(plain, want0) and not _same(want0, want1)

    m.set_dropout_rng_state((True, seed, 0))
    got0 = net.forward(x, eps, None)
    assert _same(got0, want0) and m.get_dropout_rng_state() == (True, seed, 504)
    assert torch.equal(net.backward(d), g0)
    got1 = net.forward(x, eps, None)                            # the next range of the stream
    assert _same(got1, want1) and m.get_dropout_rng_state() == (True, seed, 1008)
    assert torch.equal(net.backward(d), g1) and not torch.equal(g0, g1)

    # an explicit mask is used as before and does not advance the stream; nor does eval mode, nor encode
    assert _same(net.forward(x, eps, mask(0)), want0) and m.get_dropout_rng_state()[2] == 1008
    net.forward(x, eps, None, train=0)
    assert m.get_dropout_rng_state()[2] == 1008
    m.encode(x)
    assert m.get_dropout_rng_state()[2] == 1008

    # the module path and Trainer.step leave the mask to the engine while the stream is on
    m.set_dropout_rng_state((True, seed, 0))
    out = m(x, eps=eps)
    assert torch.equal(out[0].detach(), want0["recon"]) and m.get_dropout_rng_state()[2] == 504

    # decode: the same layout (the decoder blocks read their part), the same advance
    z = torch.randn(B, 5, generator=g).cuda()
    m.set_dropout_rng_state((True, seed, 4096))
    want_dec = net.decode(z, mask(4096))
    assert m.get_dropout_rng_state()[2] == 4096
    assert torch.equal(net.decode(z, None), want_dec) and m.get_dropout_rng_state()[2] == 4096 + 504
    assert torch.equal(m.decode(z), net.decode(z, mask(4096 + 504)))
    assert m.get_dropout_rng_state()[2] == 4096 + 1008
    net.decode(z, None, train=0)
    assert m.get_dropout_rng_state()[2] == 4096 + 1008

    # off again: NULL means no dropout, the position is kept
    m.set_dropout_rng_state((False, seed, 4096 + 1008))
    assert _same(net.forward(x, eps, None), plain) and m.get_dropout_rng_state() == (False, seed, 4096 + 1008)
    torch.cuda.synchronize()
    L.check_device("engine draw")


def test_other_nets_have_no_dropout_stream(cuda):
    ae = hlmc_amd.SimpleAutoencoder(13, 6).cuda()
    on, seed, off = C.c_int(), C.c_uint64(), C.c_uint64()
    h = ae._native_net().h
    assert L.lib().hlmc_net_set_dropout_rng(h, 1, 3, 0) == -3
    assert L.lib().hlmc_net_get_dropout_rng(h, C.byref(on), C.byref(seed), C.byref(off)) == -3


def test_trainer_step_writes_its_sums_where_told(cuda):
    """sums= redirects the loss sums (same bits as the default buffer gets); a wrong destination is refused."""
    a, b = _model(SMALL, 2), _model(SMALL, 2)
    ta, tb = hlmc_amd.Trainer(a), hlmc_amd.Trainer(b)
    g = torch.Generator().manual_seed(1)
    x, eps = torch.randn(6, 37, generator=g).cuda(), torch.randn(6, 5, generator=g).cuda()
    mask = a.make_dropout_mask(6, cuda)
    table = torch.full((4, 3), -7.0, dtype=torch.float64, device=cuda)
    default = ta.step(x, eps=eps, dropout=mask)
    out = tb.step(x, eps=eps, dropout=mask, sums=table[2])
    assert out.data_ptr() == table[2].data_ptr()
    assert torch.equal(table[2], default) and bool((table[[0, 1, 3]] == -7.0).all())
    for bad in (table[:, 0], table[2].float(), table[2][:2], table[2].cpu()):
        with pytest.raises(ValueError):
            tb.step(x, eps=eps, dropout=mask, sums=bad)
    ta.release()
    tb.release()


# ------------------------------------------------------------------------------------------------ epoch means
@pytest.mark.parametrize("nb", [1, 3, 42])
def test_vae_epoch_means_equals_the_restatement(cuda, nb):
    rng = np.random.default_rng(nb)
    sums = np.stack([rng.uniform(1e3, 2e4, nb), rng.uniform(-1, 1, nb), -rng.uniform(10, 900, nb)], axis=1)
    na_nl = np.array([[32 * 370, 32 * 32]] * (nb - 1) + [[11 * 370, 11 * 32]], dtype=np.int64)
    out = torch.full((5,), -3.0, dtype=torch.float64, device=cuda)
    dsums, dn = torch.from_numpy(sums).cuda(), torch.from_numpy(na_nl).cuda()
    L.check(L.lib().hlmc_vae_epoch_means(L.stream(), dsums.data_ptr(), dn.data_ptr(), nb, 0.8, out.data_ptr() + 8))
    got = out.cpu().tolist()
    assert got[0] == -3.0 and got[4] == -3.0
    assert tuple(got[1:4]) == FC.epoch_means(sums.tolist(), na_nl.tolist(), 0.8)


# ------------------------------------------------------------------------------------------------ the whole fit
STOP = dict(epochs=60, patience=3, lr_patience=1, lr=1e-2)
RUNS = {"stops": STOP, "four epochs": dict(epochs=4), "last weights": dict(**STOP, restore_best=False)}
SEED = 42
_fits = {}


def _fit_pair(cfg, run):
    """fit_vae and the hand loop from identical models, data and generators; computed once per case."""
    key = (cfg[0], run)
    if key not in _fits:
        X = _data(75, cfg[0])
        a, b = _model(cfg, SEED), _model(cfg, SEED)
        res = hlmc_amd.fit_vae(a, X, generator=torch.Generator().manual_seed(9), **RUNS[run])
        hand = FC.hand_loop(b, X, generator=torch.Generator().manual_seed(9), **RUNS[run])
        torch.cuda.synchronize()
        _fits[key] = (a, b, res, hand, X)
    return _fits[key]


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("cfg", [SMALL, REFSHAPE], ids=["small", "reference shape"])
def test_fit_vae_equals_the_hand_loop(cuda, cfg, run):
    """n = 75 at batch 32: two full batches and a tail of 11 per epoch."""
    a, b, res, hand, _ = _fit_pair(cfg, run)
    hh = hand["history"]
    print(f"\n{cfg[0]}-d {run}: epochs run {len(hh['loss'])}, best {hand['best_epoch']}, stopped "
          f"{hand['stopped_epoch']}, lr {sorted(set(hh['lr'].tolist()), reverse=True)}, loss {hh['loss'][0]:.6g} -> "
          f"{hh['loss'].min():.6g}")
    if "patience" in RUNS[run]:   # on the HAND LOOP's record: otherwise the comparison is vacuous
        assert hand["stopped_epoch"] is not None and hand["stopped_epoch"] < 59
        assert hh["lr"].min() <= 0.5e-2 and hh["lr"][0] == 1e-2
        assert hand["best_epoch"] == hand["stopped_epoch"] - 3
    else:
        assert hand["stopped_epoch"] is None and len(hh["loss"]) == 4
    assert np.isfinite(hh["loss"]).all()
    for k in ("loss", "recon", "kl", "lr"):
        assert res.history[k].dtype == np.float64
        np.testing.assert_array_equal(res.history[k], hh[k], err_msg=k)
    assert res.best_epoch == hand["best_epoch"] and res.stopped_epoch == hand["stopped_epoch"]
    assert res.best_loss == hand["best_loss"] == hh["loss"][hand["best_epoch"]]
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) == list(res.best_state) == list(hand["best_state"])
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
        assert torch.equal(res.best_state[k], hand["best_state"][k]) and res.best_state[k].dtype == sa[k].dtype, k
    restored = all(torch.equal(sa[k], res.best_state[k]) for k in sa)
    assert restored == RUNS[run].get("restore_best", True) or hand["best_epoch"] == len(hh["loss"]) - 1
    steps = 3 * len(hh["loss"])
    assert int(sa["encoder.1.num_batches_tracked"]) == (3 * (hand["best_epoch"] + 1) if restored else steps)
    assert res.eps_rng == hand["eps_rng"] and res.dropout_rng == hand["dropout_rng"]
    nl, nm = cfg[2], sum(a.mask_widths())
    per_epoch = lambda w: 2 * FC.round4(32 * w) + FC.round4(11 * w)
    assert res.eps_rng[1] == len(hh["loss"]) * per_epoch(nl) and res.dropout_rng[1] == len(hh["loss"]) * per_epoch(nm)
    assert a.training and a.get_dropout_rng_state() == (False, *res.dropout_rng)


def test_latents_after_the_fit_are_the_best_states(cuda):
    """The engine must see the restored weights: a fresh model that loads best_state gives the same latents, bit for
    bit (stale packed weights -- a restore the engine did not notice -- would give the last epoch's)."""
    a, _, res, hand, X = _fit_pair(REFSHAPE, "stops")
    assert hand["best_epoch"] < len(hand["history"]["loss"]) - 1       # best and last weights differ
    fresh = _model(REFSHAPE, 1)
    fresh.load_state_dict(res.best_state)
    was = a.training
    a.eval()
    fresh.eval()
    za, zf = a.get_latent_features(X), fresh.get_latent_features(X)
    a.train(was)
    assert za.shape == (75, 32) and torch.equal(za, zf)
    last, _, _, _, _ = _fit_pair(REFSHAPE, "last weights")
    last.eval()
    zl = last.get_latent_features(X)
    last.train()
    assert not torch.equal(zl, za)


def test_second_fit_continues_both_streams(cuda):
    m = _model(SMALL, 4)
    X = _data(75, 37)
    r1 = hlmc_amd.fit_vae(m, X, epochs=1)
    r2 = hlmc_amd.fit_vae(m, X, epochs=1)
    assert r2.eps_rng == (r1.eps_rng[0], 2 * r1.eps_rng[1]) and r2.dropout_rng == (r1.dropout_rng[0], 2 * r1.dropout_rng[1])
    r3 = hlmc_amd.fit_vae(m, X, epochs=1, dropout_seed=5)
    assert r3.dropout_rng == (5, r1.dropout_rng[1])


# ------------------------------------------------------------------------------------------------ the oracle
def _oracle_epochs(dtype, X, orders, eps_list, masks_list, widths, lr=1e-4, beta=0.8):
    """Epochs of the reference loop through oracle/models_oracle.py's VAE with torch.optim.Adam on the CPU in `dtype`,
    on the rows, eps and dropout masks the engine used; the nn.Dropout modules patched as tests/test_models_gpu.py does.
    Returns per epoch (loss, recon, kl): means of the per-step .item() values."""
    torch.manual_seed(SEED)
    ora = OM.VAE(SMALL[0], list(SMALL[1]), SMALL[2]).to(dtype)
    opt = torch.optim.Adam(ora.parameters(), lr=lr)
    state = {}

    def hook(mod, inp, out):
        m = next(state["it"])
        return inp[0] * m.to(inp[0].dtype) / 0.8

    hooks = [mod.register_forward_hook(hook) for mod in ora.modules() if isinstance(mod, torch.nn.Dropout)]
    ora.train()
    X = X.to(dtype)
    out, step = [], 0
    for order in orders:
        ep = [0.0, 0.0, 0.0]
        nb = (len(order) + 31) // 32
        for k in range(nb):
            x = X[order[32 * k:32 * (k + 1)]]
            B = x.shape[0]
            flat, cuts, o = masks_list[step], [], 0
            for w in widths:
                cuts.append(torch.from_numpy(flat[o:o + B * w].reshape(B, w).astype(np.float64)))
                o += B * w
            state["it"] = iter(cuts)
            r, mu, lv, _ = ora(x, eps=eps_list[step].to(dtype))
            loss = OM.vae_loss(r, x, mu, lv, beta=beta)
            opt.zero_grad()
            loss[0].backward()
            opt.step()
            for i in range(3):
                ep[i] += loss[i].item()
            step += 1
        out.append(tuple(v / nb for v in ep))
    for h in hooks:
        h.remove()
    return out


def test_two_epochs_against_the_float64_oracle(cuda):
    """Two epochs of the small case (six Adam steps): each epoch's loss, recon and kl within
    4 x |float32 oracle - float64 oracle| + 1e-6 |value| of the float64 oracle's (the 1e-6 is the per-step figure of
    test_simple_vae_trainer_equals_autograd_path).  Measured on the MI355X (error / bound, printed per value): worst
    0.024 (epoch 0 kl: |err| 7.8e-9 against a bound of 3.2e-7); loss and recon at 0.010."""
    from hlmc_amd.train import dataloader_order
    X = _data(75, 37)
    m = _model(SMALL, SEED)
    seed_eps, off_eps = m.get_rng_state()
    res = hlmc_amd.fit_vae(m, X, epochs=2, generator=torch.Generator().manual_seed(9))
    seed_drop = res.dropout_rng[0]
    g = torch.Generator().manual_seed(9)
    orders = [dataloader_order(75, g) for _ in range(2)]
    widths = m.mask_widths()
    eps_list, masks_list, off_drop = [], [], 0
    for _ in range(2):
        for B in (32, 32, 11):
            e = torch.empty(B, 5, device=cuda)
            L.check(L.lib().hlmc_randn(L.stream(), e.data_ptr(), B * 5, seed_eps, off_eps))
            eps_list.append(e.cpu())
            off_eps += FC.round4(B * 5)
            masks_list.append(FC.keep_mask(B * sum(widths), 0.2, seed_drop, off_drop))
            off_drop += FC.round4(B * sum(widths))
    assert (seed_eps, off_eps) == res.eps_rng and (seed_drop, off_drop) == res.dropout_rng
    Xc = X.cpu()
    o64 = _oracle_epochs(torch.float64, Xc, orders, eps_list, masks_list, widths)
    o32 = _oracle_epochs(torch.float32, Xc, orders, eps_list, masks_list, widths)
    worst = 0.0
    for e in range(2):
        for i, k in enumerate(("loss", "recon", "kl")):
            got, want = float(res.history[k][e]), o64[e][i]
            bound = 4 * abs(o32[e][i] - want) + 1e-6 * abs(want)
            ratio = abs(got - want) / bound
            worst = max(worst, ratio)
            print(f"\nepoch {e} {k}: engine {got:.12g} oracle64 {want:.12g} oracle32 {o32[e][i]:.12g} "
                  f"|err| {abs(got - want):.3e} bound {bound:.3e} ratio {ratio:.3f}")
    print(f"\nworst ratio {worst:.3f}")
    for e in range(2):
        for i, k in enumerate(("loss", "recon", "kl")):
            want = o64[e][i]
            assert abs(float(res.history[k][e]) - want) <= 4 * abs(o32[e][i] - want) + 1e-6 * abs(want), (e, k)


# ------------------------------------------------------------------------------------------------ the table
def test_simple_vae_experiment_on_three_blobs(cuda):
    rng = np.random.default_rng(0)
    centres = 6.0 * rng.standard_normal((3, 20))
    feats = np.concatenate([c + rng.standard_normal((50, 20)) for c in centres]).astype(np.float32)
    # PCA keeps at most 20 components of 20 features: a latent width of 8 instead of the script's 32
    out = hlmc_amd.simple_vae_experiment(feats, hidden_dims=(32, 16), latent_dim=8, epochs=5)
    assert out["latents"].shape == (150, 8) and out["latents"].is_cuda and out["best_k"] in (3, 5, 7, 9)
    assert len(out["fit"].history["loss"]) == 5 and not out["model"].training
    rows = out["rows"]
    assert [r["Method"] for r in rows] == ["VAE + KMeans", "PCA + KMeans"]
    for r in rows:
        assert list(r) == ["Method", "Silhouette", "Calinski-Harabasz", "Architecture"]
        assert r["Architecture"] == "Simple VAE"
        assert np.isfinite(r["Silhouette"]) and np.isfinite(r["Calinski-Harabasz"]) and -1 <= r["Silhouette"] <= 1
    want = hlmc_amd.KMeans(n_clusters=out["best_k"], random_state=42, n_init=10).fit_predict(out["latents"])
    np.testing.assert_array_equal(out["vae_labels"], want)
    assert rows[0]["Silhouette"] == hlmc_amd.metrics.silhouette_score(out["latents"], want)
    assert rows[0]["Calinski-Harabasz"] == hlmc_amd.metrics.calinski_harabasz_score(out["latents"], want)
    _, pca_labels, pca_scores = hlmc_amd.pca_kmeans_baseline(feats, 8, out["best_k"])
    np.testing.assert_array_equal(out["pca_labels"], pca_labels)
    assert rows[1]["Silhouette"] == pca_scores["Silhouette"]
    assert rows[1]["Calinski-Harabasz"] == pca_scores["Calinski-Harabasz"]
    # the latents are those of a model holding the fit's best weights
    fresh = _model((20, [32, 16], 8), 1)
    fresh.load_state_dict(out["fit"].best_state)
    fresh.eval()
    assert torch.equal(fresh.get_latent_features(torch.from_numpy(feats).cuda()), out["latents"])


def test_graph_mode_step_keeps_the_stream_out_of_the_graph(cuda):
    """The stream's offset is host-side state passed to the launch by value: recorded into a graph it would replay one
    mask.  In graph mode (GraphedStep's flag) Trainer.step therefore draws the mask with torch, as it does eps, and the
    engine's stream does not move; back in eager mode the engine draws again."""
    m = _model(SMALL, 6)
    tr = hlmc_amd.Trainer(m)
    x = _data(8, 37)
    m.set_dropout_rng_state((True, 77, 0))
    tr._graph = True
    tr.prepare_step_coefficients()
    tr.step(x)
    assert m.get_dropout_rng_state() == (True, 77, 0) and m.get_rng_state()[1] == 0
    tr._graph = False
    tr.step(x)
    assert m.get_dropout_rng_state() == (True, 77, FC.round4(8 * 72)) and m.get_rng_state()[1] == FC.round4(8 * 5)
    tr.release()
    m.set_dropout_rng_state((False, 77, 0))
    torch.cuda.synchronize()
