"""SimpleAutoencoder (src/Conditional_VAE.py:252-273) on the MI355X against oracle/models_oracle.SimpleAutoencoder in
float64 on the CPU: the engine's kind 3 (forward / encode / decode / backward), hlmc_batch_gather, hlmc_mse_rows, the
padded train step, Adam, the whole fit (graphed and eager), bf16 mode and the K-Means baseline row.

Tolerances (all set before the code ran):
  * outputs: relative L2 error <= 1e-4, the project's contract (tests/test_models_gpu.py, `rel` as defined there);
  * gradients: relative L2 error of every tensor against the float64 oracle <= TOL_GRAD = 1e-3, compare_step's
    tol_grad in tests/test_models_gpu.py (taken plainly: without its 8 x fp32-oracle and kink-envelope allowances);
  * hlmc_mse_rows: the counted rounding bounds of tests/ae_check.py;
  * Adam trajectories: the form of test_three_adam_steps_match_fixture_trajectory (every entry within 2 lr steps,
    and the fraction within 1e-2 lr at least the float64 oracle chain's own fraction less 0.10, capped at 0.90 --
    0.97 / less 0.03 after the first step);
  * bf16: 3 x the error recorded on the MI355X + 0.01 (tests/golden/ae_bf16_err.json), against the oracle.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, TensorDataset

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import models_oracle as OM
from tests import ae_check as AE

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4    # tests/test_models_gpu.py: the output contract
TOL_GRAD = 1e-3   # tests/test_models_gpu.py compare_step: tol_grad
DIMS = [(290, 64), (13, 6), (8, 64), (1, 1)]
HIDDEN = ("encoder.0", "encoder.2", "decoder.0", "decoder.2")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def build(D, Lz, dtype="fp32", seed=42, dead=False):
    """(float32 oracle on the CPU, ours on the GPU) from the same seed.  dead: half of every hidden layer's units get a
    bias of -5 (pre-activations are O(1)), so they are dead for every row and their ReLU mask is all zero."""
    torch.manual_seed(seed)
    ora = OM.SimpleAutoencoder(D, Lz)
    if dead:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name in HIDDEN:
                b = ora.get_submodule(name).bias
                b.copy_(torch.where(torch.rand(b.shape, generator=g) < 0.5, torch.full_like(b, -5.0), b))
    torch.manual_seed(seed)
    ours = hlmc_amd.SimpleAutoencoder(D, Lz, compute_dtype=dtype)
    ours.load_state_dict(ora.state_dict())
    return ora, ours.cuda()


def data(B, D, seed=0):
    return torch.randn(B, D, generator=torch.Generator().manual_seed(100 * B + D + seed))


@pytest.fixture(autouse=True)
def _clear_status():
    L.lib().hlmc_device_status(1)
    yield
    assert L.lib().hlmc_device_status(1) == 0


# ------------------------------------------------------------------ forward / encode / decode
@pytest.mark.parametrize("B", [1, 24, 32, 33, 64])
@pytest.mark.parametrize("D,Lz", DIMS)
def test_forward_encode_decode_match_oracle(cuda, D, Lz, B):
    ora, ours = build(D, Lz)
    ora64 = ora.double()
    x = data(B, D)
    zin = data(B, Lz, seed=1)
    with torch.no_grad():
        ro, zo = ora64(x.double())
        do = ora64.decoder(zin.double())
        for train in (True, False):   # no BatchNorm: the same values, and train mode takes B = 1
            ours.train(train)
            r, z = ours(x.cuda())
            ze, d = ours.encode(x.cuda()), ours.decode(zin.cuda())
            torch.cuda.synchronize()
            errs = dict(recon=rel(r, ro), z=rel(z, zo), encode=rel(ze, zo), decode=rel(d, do))
            print(f"D={D} L={Lz} B={B} train={train}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            assert max(errs.values()) <= TOL_OUT, errs
            assert torch.equal(ze, z)
    assert r.shape == (B, D) and z.shape == (B, Lz)


def _native_step(ours, x, d_recon, d_z, ws):
    """hlmc_net_forward + hlmc_net_backward on the caller's workspace; returns (recon, z, flat grads)."""
    net = ours._native_net()
    B = x.shape[0]
    recon = torch.empty(B, ours.input_dim, device=x.device)
    z = torch.empty(B, ours.latent_dim, device=x.device)
    lib, s = L.lib(), L.stream()
    L.check(lib.hlmc_net_forward(net.h, s, B, 1, L.ptr(x), None, None, None, None, L.ptr(recon), None, None, None,
                                 L.ptr(z), ws.data_ptr()), "hlmc_net_forward")
    L.check(lib.hlmc_net_backward(net.h, s, B, L.ptr(d_recon), None, L.ptr(d_z), None, ws.data_ptr()),
            "hlmc_net_backward")
    L.check(lib.hlmc_net_settle(net.h, s))
    torch.cuda.synchronize()
    return recon, z, ours._gflat.clone()


def test_padding_columns_do_not_leak_from_a_poisoned_workspace(cuda):
    """D = 13 and L = 6 are padded to leading dimensions 16 and 8: with the workspace NaN-filled before the call the
    outputs and every gradient are finite and equal, bit for bit, those of a zero-filled workspace."""
    _, ours = build(13, 6)
    B = 33
    x, dr, dz = data(B, 13).cuda(), data(B, 13, seed=2).cuda(), data(B, 6, seed=3).cuda()
    nbytes = ours._native_net().workspace_bytes(B)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    clean = _native_step(ours, x, dr, dz, ws)
    ws.view(torch.float32)[:] = float("nan")
    poisoned = _native_step(ours, x, dr, dz, ws)
    for a, b in zip(clean, poisoned):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def test_engine_refuses_what_kind3_has_no_use_for(cuda):
    """The NULL rules of include/hlmc.h for kind 3, checked on the host: nothing is launched (the outputs keep
    their fill)."""
    _, ours = build(13, 6)
    net, lib, s = ours._native_net(), L.lib(), L.stream()
    B = 4
    x, t = data(B, 13).cuda(), torch.zeros(B, 13, device="cuda")
    recon, z = torch.full((B, 13), 7.0, device="cuda"), torch.full((B, 6), 7.0, device="cuda")
    ws = torch.zeros(net.workspace_bytes(B), dtype=torch.uint8, device="cuda")
    p = L.ptr
    fwd = lambda **k: lib.hlmc_net_forward(net.h, s, B, 1, p(x), k.get("in1"), None, k.get("eps"), k.get("drop"),
                                           p(recon), None, k.get("mu"), k.get("lv"), p(z), ws.data_ptr())
    for bad in (dict(in1=p(t)), dict(eps=p(t)), dict(drop=p(t)), dict(mu=p(t)), dict(lv=p(t))):
        assert fwd(**bad) == -1, bad
    assert lib.hlmc_net_encode(net.h, s, B, 0, p(x), None, None, p(z), p(t), ws.data_ptr()) == -1
    torch.cuda.synchronize()
    assert float(recon.min()) == 7.0 and float(z.min()) == 7.0
    assert fwd() == 0
    assert lib.hlmc_net_backward(net.h, s, B, p(t), p(t), None, None, ws.data_ptr()) == -1   # d_recon_text
    assert lib.hlmc_net_backward(net.h, s, B, p(t), None, None, p(t), ws.data_ptr()) == -1   # d_logvar
    assert lib.hlmc_net_backward(net.h, s, B, p(t), None, None, None, ws.data_ptr()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("dead", [False, True], ids=["init", "half_dead"])
@pytest.mark.parametrize("mode", ["recon", "z", "both"])
@pytest.mark.parametrize("D,Lz,B", [(290, 64, 32), (13, 6, 33), (8, 64, 1)])
def test_backward_matches_float64_oracle(cuda, D, Lz, B, mode, dead):
    """Upstream gradients on recon only, on z only (the engine's d_mu slot) and on both, through the nn.Module path."""
    ora, ours = build(D, Lz, dead=dead)
    ora64 = ora.double()
    x, wr, wz = data(B, D), data(B, D, seed=5), data(B, Lz, seed=6)

    def loss(r, z, wr, wz):
        return (r * wr).sum() * (mode != "z") + (z * wz).sum() * (mode != "recon")

    ro, zo = ora64(x.double())
    loss(ro, zo, wr.double(), wz.double()).backward()
    if dead:
        # about half of the units carry the -5 bias, and every one of them is dead for every row of the batch
        forced = ora64.encoder[0].bias == -5.0
        h = torch.relu(ora64.encoder[0](x.double())).detach()
        assert 0.4 < float(forced.double().mean()) < 0.6 and float(h[:, forced].max()) == 0.0
        assert float(h[:, ~forced].max()) > 0.0
    ours.train()
    r, z = ours(x.cuda())
    loss(r, z, wr.cuda(), wz.cuda()).backward()
    torch.cuda.synchronize()
    worst = 0.0
    for (name, po), pm in zip(ora64.named_parameters(), ours.parameters()):
        assert pm.grad is not None, name
        if po.grad is None or float(po.grad.abs().max()) == 0.0:   # the decoder under a loss on z alone
            assert float(pm.grad.abs().max()) == 0.0, name
            continue
        e = rel(pm.grad, po.grad)
        worst = max(worst, e)
        assert e <= TOL_GRAD, f"grad {name}: {e:.3e}"
    print(f"D={D} L={Lz} B={B} {mode} dead={dead}: worst gradient rel {worst:.2e}")


# ------------------------------------------------------------------ hlmc_batch_gather
def _gather(X, idx, count, B):
    n, d = X.shape
    out = torch.full((B, d), float("nan"), device="cuda")
    valid = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    L.check(L.lib().hlmc_batch_gather(L.stream(), X.data_ptr(), n, d, idx.data_ptr(), count, B, out.data_ptr(),
                                      valid.data_ptr()), "hlmc_batch_gather")
    torch.cuda.synchronize()
    return out, int(valid.item())


@pytest.mark.parametrize("d", [1, 3, 290, 512, 1030, 4100])
def test_batch_gather_is_bit_equal_to_indexing(cuda, d):
    """d % 4 != 0 takes the 4-byte path, 512 and 4100 the float4 path; 1030 and 4100 span more than one column block."""
    B = 8
    g = torch.Generator().manual_seed(d)
    for n in (50, 1):
        X = torch.randn(n, d, generator=g).cuda()
        for count in (1, B - 1, B):
            idx = torch.randint(0, n, (count,), generator=g)
            idx[-1] = idx[0]                                   # a repeated row
            out, valid = _gather(X, idx.cuda(), count, B)
            want = torch.zeros(B, d, device="cuda")
            want[:count] = X[idx.cuda()]
            assert valid == count
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (n, count)


@pytest.mark.parametrize("bad", [50, -1, 2 ** 40])
def test_batch_gather_never_reads_an_index_out_of_range(cuda, bad):
    """The row of an index outside [0, n) is zeros, the others are gathered, and bit 1 of the device status word is
    raised (hlmc_net_backward then returns HLMC_EDEVICE until it is cleared)."""
    X = torch.randn(50, 13, generator=torch.Generator().manual_seed(3)).cuda()
    idx = torch.tensor([4, bad, 49, 0])
    out, valid = _gather(X, idx.cuda(), 4, 6)
    assert valid == 4
    assert torch.equal(out[[0, 2, 3]], X[[4, 49, 0]]) and float(out[1].abs().max()) == 0 and float(out[4:].abs().max()) == 0
    assert L.lib().hlmc_device_status(0) == 2
    with pytest.raises(L.HLMCError, match="hlmc_batch_gather"):
        L.check_device("gather")
    assert L.lib().hlmc_device_status(1) == 2 and L.lib().hlmc_device_status(0) == 0


# ------------------------------------------------------------------ hlmc_mse_rows
def _mse(recon, target, valid, acc, calls=1):
    B, d = recon.shape
    lib = L.lib()
    g = torch.full((B, d), float("nan"), device="cuda")
    sums = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.zeros(int(lib.hlmc_mse_rows_workspace(B, d)), dtype=torch.uint8, device="cuda")
    vd = torch.tensor([valid], dtype=torch.int32, device="cuda")
    for _ in range(calls):
        L.check(lib.hlmc_mse_rows(L.stream(), recon.data_ptr(), target.data_ptr(), B, d, vd.data_ptr(), g.data_ptr(),
                                  sums.data_ptr(), L.ptr(acc), ws.data_ptr()), "hlmc_mse_rows")
    torch.cuda.synchronize()
    return g.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("B,d,valid", AE.MSE_CASES)
def test_mse_rows_within_counted_roundings(cuda, B, d, valid):
    """d_recon within one float32 rounding of the float64 value on the valid rows and +0.0f bit for bit on the others
    although recon holds NaN there; sums2[0] within the counted float64 bound, sums2[1] exact (tests/ae_check.py
    derives both bounds and counts the roundings); acc accumulates over three calls; two runs give the same bits."""
    recon, target = AE.mse_inputs(B, d)
    recon[valid:] = np.nan
    r, t = torch.from_numpy(recon).cuda(), torch.from_numpy(target).cuda()
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    g, sums = _mse(r, t, valid, acc, calls=3)
    worst = AE.check_mse(recon, target, valid, g, sums)
    print(f"B={B} d={d} valid={valid}: worst |err| / bound of d_recon {worst:.3f}")
    m = sums[0] / sums[1]
    assert float(acc.item()) == (m + m) + m
    g2, sums2 = _mse(r, t, valid, None)
    assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and np.array_equal(sums, sums2)
    want = F.mse_loss(torch.from_numpy(recon[:valid]).double(), torch.from_numpy(target[:valid]).double())
    assert abs(m - float(want)) <= 1e-12 * float(want)


# ------------------------------------------------------------------ the train step
def _grads(model):
    out, off = {}, 0
    for n, p in model.named_parameters():
        out[n] = model._gflat[off:off + p.numel()].view_as(p).clone()
        off += p.numel()
    return out


def test_padded_step_is_the_short_step(cuda):
    """One trainer step at B = 32 with valid = 24 against a native B = 24 step: both hold the float64 oracle's 24-row
    gradients at TOL_GRAD and its loss at 1e-4, and the padded step's gradients do not move when its 8 padding rows are
    replaced by other (finite) values."""
    D, Lz = 290, 64
    ora, _ = build(D, Lz)
    ora64 = ora.double()
    x = data(32, D)
    ro, _ = ora64(x[:24].double())
    lo = F.mse_loss(ro, x[:24].double())
    lo.backward()
    valid = torch.tensor([24], dtype=torch.int32, device="cuda")
    runs = {}
    for tag in ("zeros", "noise", "short"):
        _, ours = build(D, Lz)
        ours.train()
        tr = hlmc_amd.AutoencoderTrainer(ours)
        xb = x.clone()
        xb[24:] = 0.0 if tag == "zeros" else 3.0 * data(8, D, seed=9)
        sums = tr.step(xb[:24].cuda().contiguous()) if tag == "short" else tr.step(xb.cuda(), valid)
        loss = tr.loss(sums)
        runs[tag] = _grads(ours)
        assert abs(loss - float(lo)) <= 1e-4 * float(lo), (tag, loss, float(lo))
        assert float(tr.loss_acc.item()) == loss
        tr.release()
    for name, po in ora64.named_parameters():
        for tag in ("zeros", "short"):
            e = rel(runs[tag][name], po.grad)
            assert e <= TOL_GRAD, f"{tag} grad {name}: {e:.3e}"
        assert torch.equal(runs["zeros"][name], runs["noise"][name]), name


def _traj_check(ours_params, ref_params, f64_params, lr, steps, first):
    """The tolerance form of tests/test_models_gpu.py test_three_adam_steps_match_fixture_trajectory on every entry."""
    d = torch.cat([(a.detach().cpu() - b.detach()).abs().reshape(-1) for a, b in zip(ours_params, ref_params)])
    y = torch.cat([(a.detach().float() - b.detach()).abs().reshape(-1) for a, b in zip(f64_params, ref_params)])
    frac, yard = float((d <= 1e-2 * lr).double().mean()), float((y <= 1e-2 * lr).double().mean())
    bar = min(0.97, yard - 0.03) if first else min(0.90, yard - 0.10)
    print(f"after {steps} steps: max |diff| {float(d.max()):.2e} (cap {2 * lr * steps:.1e}); {frac:.3f} within 1e-2 lr "
          f"(float64 oracle {yard:.3f}, bar {bar:.3f})")
    assert float(d.max()) <= 2 * lr * steps + 1e-6
    assert frac >= bar


def test_three_adam_steps_and_packs(cuda):
    """Three AutoencoderTrainer steps at lr = 1e-3 against torch.optim.Adam on the oracle (fp32, CPU), the float64
    oracle chain as the yardstick; then the packs Adam wrote against fresh packs of the same weights, bit for bit, as
    tests/test_trainer_gpu.py test_adam_written_packs_equal_fresh_packs does."""
    D, Lz, B, lr = 290, 64, 32, 1e-3
    ora, ours = build(D, Lz)
    ora64 = build(D, Lz)[0].double()
    opt, opt64 = torch.optim.Adam(ora.parameters(), lr=lr), torch.optim.Adam(ora64.parameters(), lr=lr)
    ours.train()
    tr = hlmc_amd.AutoencoderTrainer(ours, lr=lr)
    for step in range(3):
        x = data(B, D, seed=20 + step)
        for m, o, xx in ((ora, opt, x), (ora64, opt64, x.double())):
            o.zero_grad()
            F.mse_loss(m(xx)[0], xx).backward()
            o.step()
        tr.step(x.cuda())
        if step in (0, 2):
            torch.cuda.synchronize()
            _traj_check(list(ours.parameters()), list(ora.parameters()), list(ora64.parameters()), lr, step + 1, step == 0)
    assert tr.step_count == 3
    ours.eval()
    fresh = hlmc_amd.SimpleAutoencoder(D, Lz).cuda()
    fresh.load_state_dict(ours.state_dict())
    fresh.eval()
    x = data(B, D, seed=30).cuda()
    with torch.no_grad():
        got, want = ours(x) + (ours.encode(x),), fresh(x) + (fresh.encode(x),)
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and torch.equal(a, b)
        w = max(ours.parameters(), key=lambda p: p.numel())   # not vacuous: the trained net reads the packs Adam wrote
        w.mul_(2.0)
        again = ours(x)
        w.mul_(0.5)
    assert torch.equal(again[0], got[0])
    tr.release()


# ------------------------------------------------------------------ the whole fit
def _oracle_fit(X, D, Lz, epochs, lr, double):
    torch.manual_seed(42)
    ora = OM.SimpleAutoencoder(D, Lz)
    if double:
        ora, X = ora.double(), X.double()
    opt = torch.optim.Adam(ora.parameters(), lr=lr)
    torch.manual_seed(7)
    loader = DataLoader(TensorDataset(X), batch_size=32, shuffle=True)
    hist = []
    for _ in range(epochs):
        tot = 0.0
        for (xb,) in loader:
            opt.zero_grad()
            loss = F.mse_loss(ora(xb)[0], xb)
            loss.backward()
            opt.step()
            tot += loss.item()
        hist.append(tot / len(loader))
    return ora, np.array(hist)


def _our_fit(X, D, Lz, epochs, lr, graph):
    torch.manual_seed(42)
    m = hlmc_amd.SimpleAutoencoder(D, Lz).cuda()
    torch.manual_seed(7)
    hist = hlmc_amd.fit_autoencoder(m, X.cuda(), epochs=epochs, lr=lr, graph=graph)
    return m, hist


def test_fit_graphed_equals_eager_and_follows_the_oracle_loop(cuda):
    """n = 77 at batch 32: batches of 32, 32 and 13 rows, two epochs, six Adam steps (two eager, four replays of the
    one captured graph, the short batch among them)."""
    n, D, Lz, lr = 77, 13, 6, 1e-3
    X = data(n, D, seed=40)
    mg, hg = _our_fit(X, D, Lz, 2, lr, True)
    me, he = _our_fit(X, D, Lz, 2, lr, False)
    assert hg.dtype == np.float64 and hg.shape == (2,) and np.array_equal(hg, he)
    for (name, a), b in zip(mg.named_parameters(), me.parameters()):
        assert torch.equal(a, b), name
    ora, ho = _oracle_fit(X, D, Lz, 2, lr, False)
    ora64, _ = _oracle_fit(X, D, Lz, 2, lr, True)
    print(f"loss history ours {hg}, oracle {ho}")
    assert np.all(np.abs(hg - ho) <= 1e-4 * np.abs(ho))
    _traj_check(list(mg.parameters()), list(ora.parameters()), list(ora64.parameters()), lr, 6, False)


def test_fit_with_a_tail_of_one_row(cuda):
    n, D, Lz = 33, 13, 6
    X = data(n, D, seed=41)
    m, h = _our_fit(X, D, Lz, 2, 1e-3, True)
    _, ho = _oracle_fit(X, D, Lz, 2, 1e-3, False)
    assert np.all(np.isfinite(h)) and np.all(np.abs(h - ho) <= 1e-4 * np.abs(ho))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ------------------------------------------------------------------ bf16
BF16_FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ae_bf16_err.json")


def test_bf16_mode_tracks_the_oracle(cuda):
    """Forward and one backward (mse_loss) in bf16 mode at (290, 64), B = 32, against the float64 oracle: every output
    and gradient tensor within 3 x its error recorded on the MI355X + 0.01 (tests/golden/ae_bf16_err.json, written by a
    run of this test with HLMC_RECORD_AE_BF16=<path>), the rule of tests/golden/bf16_tensor_err.json."""
    D, Lz, B = 290, 64, 32
    ora, ours = build(D, Lz, dtype="bf16")
    ora64 = ora.double()
    x = data(B, D)
    ro, zo = ora64(x.double())
    F.mse_loss(ro, x.double()).backward()
    ours.train()
    r, z = ours(x.cuda())
    F.mse_loss(r, x.cuda()).backward()
    torch.cuda.synchronize()
    per = {"recon": rel(r, ro), "z": rel(z, zo)}
    for (name, po), pm in zip(ora64.named_parameters(), ours.parameters()):
        per["grad " + name] = rel(pm.grad, po.grad)
    print("bf16 errors: " + ", ".join(f"{k} {v:.4f}" for k, v in per.items()))
    path = os.environ.get("HLMC_RECORD_AE_BF16")
    if path:
        with open(path, "w") as f:
            json.dump({k: round(v, 6) for k, v in per.items()}, f, indent=1, sort_keys=True)
    with open(BF16_FIXTURE) as f:
        meas = json.load(f)
    assert set(meas) == set(per)
    bad = {k: (v, 3.0 * meas[k] + 0.01) for k, v in per.items() if v > 3.0 * meas[k] + 0.01}
    assert not bad, bad
    assert min(per.values()) > 1e-5   # bf16 operands really ran (fp32 mode sits near 1e-7)


# ------------------------------------------------------------------ the baseline rows
def _blobs():
    g = torch.Generator().manual_seed(11)
    centers = 6.0 * torch.randn(3, 20, generator=g)
    y = torch.arange(300) % 3
    return (centers[y] + torch.randn(300, 20, generator=g)), y.numpy()


def test_autoencoder_kmeans_baseline_separates_blobs(cuda):
    X, y = _blobs()
    feats, labels, scores, hist = hlmc_amd.autoencoder_kmeans_baseline(X, 8, 3, y_true=y, epochs=5)
    assert feats.is_cuda and feats.shape == (300, 8) and feats.dtype == torch.float32
    assert set(scores) == {"Silhouette", "Calinski-Harabasz", "NMI", "ARI", "Purity"}
    print(f"autoencoder + K-Means on blobs: {scores}, loss {hist}")
    assert scores["ARI"] == 1.0
    assert hist.shape == (5,) and hist.dtype == np.float64 and hist[-1] < hist[0]
    f2, l2, s2 = hlmc_amd.direct_kmeans_baseline(X, 3, y_true=y)
    assert f2.shape == (300, 20) and set(s2) == set(scores) and s2["ARI"] == 1.0
    _, _, s3 = hlmc_amd.pca_kmeans_baseline(X, 2, 3)
    assert set(s3) == {"Silhouette", "Calinski-Harabasz"}
