"""fit_vae (the Simple VAE training run of src/Simple_VAE.py:131-226 and its table, :240-295), the parts that need no
GPU: the plateau rules against live torch, the host restatement of the dropout stream, the host-side argument checks
of the new entry points, fit_vae's own argument errors and the consolidated CSV."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from hlmc_amd.train import PlateauStopper
from oracle import rng_oracle as RNG
from tests import fit_cases as FC

ONE = C.c_void_p(256)          # non-null placeholder: validation fails before anything is dereferenced
NULL = None


def _err():
    return L.lib().hlmc_last_error().decode()


# ------------------------------------------------------------------------------------------------ PlateauStopper
def _torch_and_counter(series, lr, factor, lr_patience, stop_patience, **kw):
    """(lr after each epoch, improved flags, first stop epoch or None) from a live ReduceLROnPlateau on a dummy
    optimizer and the reference's own counter (src/Simple_VAE.py:202-217), run over the whole series."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=factor, patience=lr_patience, **kw)
    best, counter, lrs, improved, stop = float("inf"), 0, [], [], None
    for e, v in enumerate(series):
        sched.step(v)
        if v < best:
            best, counter = v, 0
            improved.append(True)
        else:
            counter += 1
            improved.append(False)
        lrs.append(float(opt.param_groups[0]["lr"]))
        if counter >= stop_patience and stop is None:
            stop = e
    return lrs, improved, stop


def _ours(series, lr, factor, lr_patience, stop_patience, **kw):
    st = PlateauStopper(lr, factor=factor, lr_patience=lr_patience, stop_patience=stop_patience, **kw)
    lrs, improved, stop = [], [], None
    for e, v in enumerate(series):
        imp, new_lr, s = st.update(v)
        lrs.append(new_lr)
        improved.append(imp)
        if s and stop is None:
            stop = e
    return lrs, improved, stop, st


def test_plateau_stopper_on_the_slow_descent_series():
    """[1, .9, .8, .7, .6], forty improvements of 1e-5 relative (under the scheduler's 1e-4 threshold, over the
    stopper's strict <), then thirty repeats: torch halves the rate at epoch 53, the run stops at epoch 59, best
    epoch 44 (0-based)."""
    series = FC.slow_descent_series()
    assert len(series) == 75
    want_lr, want_imp, want_stop = _torch_and_counter(series, 1e-4, 0.5, 15, 15)
    halved = [e for e in range(1, len(series)) if want_lr[e] != want_lr[e - 1]]
    assert halved[0] == 53 and want_lr[52] == 1e-4 and want_lr[53] == 5e-5      # live torch
    assert want_stop == 59
    lrs, imp, stop, st = _ours(series, 1e-4, 0.5, 15, 15)
    assert lrs == want_lr and imp == want_imp and stop == want_stop == 59
    assert max(e for e, f in enumerate(imp) if f) == 44
    st2 = PlateauStopper(1e-4)
    for v in series[:60]:
        out = st2.update(v)
    assert out == (False, 5e-5, True) and st2.best_epoch == 44 and st2.best_loss == series[44]


@pytest.mark.parametrize("name,series,kw", [
    ("monotone", [1.0 / (1 + i) for i in range(80)], {}),
    ("constant", [0.37] * 40, {}),
    ("nan", [1.0, 0.5, float("nan"), 0.4] + [float("nan")] * 40, {}),
    ("all nan", [float("nan")] * 40, {}),
    ("min_lr", [1.0] * 120, dict(min_lr=3e-5)),
    ("eps", [1.0] * 120, dict(eps=3e-5)),
    ("short patience", [1.0, 0.9] + [0.95, 0.949] * 20, {}),
    ("noisy", list(np.abs(np.sin(np.arange(200) * 0.37)) + 1.0 / (1 + np.arange(200))), {}),
])
@pytest.mark.parametrize("lr_patience,stop_patience", [(15, 15), (1, 3), (0, 1), (4, 30)])
def test_plateau_stopper_follows_torch_and_the_counter(name, series, kw, lr_patience, stop_patience):
    series = [float(v) for v in series]
    want = _torch_and_counter(series, 1e-4, 0.5, lr_patience, stop_patience, **kw)
    got = _ours(series, 1e-4, 0.5, lr_patience, stop_patience, **kw)
    assert got[0] == want[0], name
    assert got[1] == want[1] and got[2] == want[2], name
    if name == "monotone":
        assert got[2] is None and len(set(got[0])) == 1
    if name == "constant" and (lr_patience, stop_patience) == (15, 15):
        assert got[2] == 15 and got[0][15] == 1e-4      # stops at 15, no halving up to there
    if name == "all nan":
        assert got[3].best_epoch is None and got[3].best_loss == float("inf")
    if name == "min_lr" and lr_patience == 1:
        assert got[0][-1] == 3e-5
    if name == "eps" and lr_patience == 1:
        assert got[0][-1] == 5e-5                         # 5e-5 -> 2.5e-5 would lower it by less than eps


def test_plateau_stopper_refuses_a_factor_of_one():
    with pytest.raises(ValueError):
        PlateauStopper(1e-4, factor=1.0)


# ------------------------------------------------------------------------------------------------ mask restatement
def test_vector_philox_reproduces_the_known_answer_blocks():
    """The numpy Philox of tests/fit_cases.py against the Random123 known-answer vectors (philox4x32_10) and, block by
    block, against oracle/rng_oracle.py."""
    assert FC.philox_words(0, [0])[0].tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert FC.philox_words(0xffffffffffffffff, [0xffffffffffffffff], hi=(0xffffffff, 0xffffffff))[0].tolist() == [
        0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert FC.philox_words(0x299f31d0a4093822, [0x85a308d3243f6a88], hi=(0x13198a2e, 0x03707344))[0].tolist() == [
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    seed = 0x0123456789abcdef
    qs = [0, 1, 2, 0xffffffff, 0x100000000, 0x100000001, 0xfffffffffffffffe]
    got = FC.philox_words(seed, qs)
    for q, row in zip(qs, got):
        assert tuple(int(x) for x in row) == RNG.philox4x32((q & 0xffffffff, q >> 32, 0, 0),
                                                            (seed & 0xffffffff, seed >> 32))


def test_mask_restatements_agree_and_the_threshold_of_0_2_is_858993460():
    assert FC.threshold(0.2) == 858993460
    assert FC.threshold(0.0) == 0 and FC.threshold(0.5) == 1 << 31
    assert FC.threshold(math.nextafter(1.0, 0.0)) == 1 << 32       # does not fit 32 bits: nothing is kept
    for n, p, seed, off in [(0, 0.2, 1, 0), (1, 0.2, 1, 0), (5, 0.2, 42, 4), (257, 0.5, 7, 4096),
                            (12, 0.2, 99, 4 * (2 ** 32 - 1)), (64, 0.0, 3, 8), (64, math.nextafter(1.0, 0.0), 3, 8)]:
        a, b = FC.keep_mask_ref(n, p, seed, off), FC.keep_mask(n, p, seed, off)
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape == (n,)
        np.testing.assert_array_equal(a, b)
    assert FC.keep_mask(64, 0.0, 3, 8).all() and not FC.keep_mask(64, math.nextafter(1.0, 0.0), 3, 8).any()
    # a window of the stream is the stream: element g does not depend on where the call starts
    whole = FC.keep_mask(600, 0.2, 42, 0)
    np.testing.assert_array_equal(FC.keep_mask(88, 0.2, 42, 512), whole[512:])


def test_drop_share_is_binomial():
    """16,384 words at p = 0.2: the dropped share within 4 sigma (sigma = sqrt(.2 * .8 / 16384) = 0.003125) of 0.2;
    0.1968 for seed 42."""
    m = FC.keep_mask(16384, 0.2, 42, 0)
    share = 1.0 - float(m.mean())
    assert abs(share - 0.2) <= 4 * math.sqrt(0.2 * 0.8 / 16384), share
    assert round(share, 4) == 0.1968


def test_epoch_means_restatement():
    sums = [(370.0 * 32 * 0.9, 0.0, -2.0 * 32 * 32 * 0.1), (370.0 * 11 * 0.5, 0.0, -2.0 * 11 * 32 * 0.3)]
    na_nl = [(370 * 32, 32 * 32), (370 * 11, 11 * 32)]
    loss, recon, kl = FC.epoch_means(sums, na_nl, 0.8)
    assert recon == (0.9 + 0.5) / 2 and kl == (0.1 + 0.3) / 2
    assert loss == ((0.9 + 0.8 * 0.1) + (0.5 + 0.8 * 0.3)) / 2


# ------------------------------------------------------------------------------------------------ host checks
MASK_OK = dict(out=ONE, n=16, p=0.2, seed=1, offset=8)


@pytest.mark.parametrize("bad", [dict(out=NULL), dict(n=-1), dict(offset=2), dict(offset=7), dict(p=-0.1), dict(p=1.0),
                                 dict(p=1.5), dict(p=float("nan"))])
def test_dropout_mask_checks_its_arguments_on_the_host(bad):
    a = {**MASK_OK, **bad}
    st = L.lib().hlmc_dropout_mask(None, a["out"], a["n"], a["p"], a["seed"], a["offset"])
    assert st == -1 and "dropout_mask" in _err()


def test_dropout_mask_of_no_elements_launches_nothing():
    assert L.lib().hlmc_dropout_mask(None, ONE, 0, 0.2, 1, 0) == 0


MEANS_OK = dict(sums=ONE, na_nl=ONE, nb=3, beta=0.8, out3=ONE)


@pytest.mark.parametrize("bad", [dict(sums=NULL), dict(na_nl=NULL), dict(out3=NULL), dict(nb=0), dict(nb=-2),
                                 dict(beta=float("nan"))])
def test_vae_epoch_means_checks_its_arguments_on_the_host(bad):
    a = {**MEANS_OK, **bad}
    st = L.lib().hlmc_vae_epoch_means(None, a["sums"], a["na_nl"], a["nb"], a["beta"], a["out3"])
    assert st == -1 and "vae_epoch_means" in _err()


def _create(kind, cfg, dtype=0):
    h = C.c_void_p()
    assert L.lib().hlmc_net_create(kind, L.i64_array(cfg), len(cfg), dtype, C.byref(h)) == 0, _err()
    return h


def test_dropout_stream_state_of_a_net():
    lib = L.lib()
    h = _create(L.NET_SIMPLE, [37, 5, 2, 24, 12])
    on, seed, off = C.c_int(7), C.c_uint64(7), C.c_uint64(7)
    assert lib.hlmc_net_get_dropout_rng(h, C.byref(on), C.byref(seed), C.byref(off)) == 0
    assert (on.value, seed.value, off.value) == (0, 0, 0)                    # off by default
    assert lib.hlmc_net_set_dropout_rng(h, 1, 0xfedcba9876543210, 4 * (2 ** 40)) == 0
    assert lib.hlmc_net_get_dropout_rng(h, C.byref(on), C.byref(seed), C.byref(off)) == 0
    assert (on.value, seed.value, off.value) == (1, 0xfedcba9876543210, 4 * (2 ** 40))
    assert lib.hlmc_net_set_dropout_rng(h, 1, 5, 6) == -1 and "multiple of 4" in _err()
    assert lib.hlmc_net_get_dropout_rng(h, C.byref(on), C.byref(seed), C.byref(off)) == 0
    assert (on.value, seed.value, off.value) == (1, 0xfedcba9876543210, 4 * (2 ** 40))   # a refused call changes nothing
    assert lib.hlmc_net_set_dropout_rng(None, 1, 5, 8) == -1
    assert lib.hlmc_net_get_dropout_rng(h, None, C.byref(seed), C.byref(off)) == -1
    assert lib.hlmc_net_set_dropout_rng(h, 0, 5, 8) == 0
    assert lib.hlmc_net_get_dropout_rng(h, C.byref(on), C.byref(seed), C.byref(off)) == 0
    assert (on.value, seed.value, off.value) == (0, 5, 8)
    lib.hlmc_net_destroy(h)


@pytest.mark.parametrize("kind,cfg", [(L.NET_AE, [290, 64]), (L.NET_HYBRID, [16, 0, 64, 64]),
                                      (L.NET_CVAE, [16, 8, 3, 64, 64])])
def test_dropout_stream_is_the_simple_kinds_alone(kind, cfg):
    lib = L.lib()
    h = _create(kind, cfg)
    on, seed, off = C.c_int(), C.c_uint64(), C.c_uint64()
    assert lib.hlmc_net_set_dropout_rng(h, 1, 5, 8) == -3 and "Simple" in _err()
    assert lib.hlmc_net_get_dropout_rng(h, C.byref(on), C.byref(seed), C.byref(off)) == -3
    lib.hlmc_net_destroy(h)


# ------------------------------------------------------------------------------------------------ fit_vae arguments
def test_fit_vae_argument_errors_come_before_any_launch():
    m = hlmc_amd.VAE(8, [8, 4], 3)
    with pytest.raises(TypeError):
        hlmc_amd.fit_vae(hlmc_amd.SimpleAutoencoder(8, 3), torch.zeros(40, 8))
    with pytest.raises(TypeError):
        hlmc_amd.fit_vae(torch.nn.Linear(8, 8), torch.zeros(40, 8))
    for n in (33, 65, 1):
        with pytest.raises(ValueError, match="batch of one row"):
            hlmc_amd.fit_vae(m, torch.zeros(n, 8))
    with pytest.raises(ValueError, match="batch of one row"):
        hlmc_amd.fit_vae(m, torch.zeros(40, 8), batch_size=1)
    with pytest.raises(ValueError, match="batch of one row"):
        hlmc_amd.fit_vae(m, torch.zeros(41, 8), batch_size=8)
    with pytest.raises(ValueError):
        hlmc_amd.fit_vae(m, torch.zeros(40, 8), epochs=0)
    with pytest.raises(ValueError):
        hlmc_amd.fit_vae(m, torch.zeros(40, 8), batch_size=0)
    with pytest.raises(ValueError, match="columns"):
        hlmc_amd.fit_vae(m, torch.zeros(40, 9))
    with pytest.raises(ValueError):
        hlmc_amd.fit_vae(m, torch.zeros(40))
    with pytest.raises(ValueError):
        hlmc_amd.fit_vae(m, torch.zeros(40, 8), patience=0)
    with pytest.raises(ValueError):
        hlmc_amd.fit_vae(m, torch.zeros(40, 8), lr_factor=1.0)
    with pytest.raises(L.HLMCError):                 # a CPU model: refused, never computed in eager torch
        hlmc_amd.fit_vae(m, torch.zeros(40, 8), epochs=1)


def test_trainer_step_keeps_its_signature_default():
    import inspect
    p = inspect.signature(hlmc_amd.Trainer.step).parameters
    assert p["sums"].default is None and list(p)[-1] == "sums"


def test_new_symbols_are_bound_and_exported():
    for s in ("hlmc_dropout_mask", "hlmc_net_set_dropout_rng", "hlmc_net_get_dropout_rng", "hlmc_vae_epoch_means"):
        assert s in L.exported_symbols() and hasattr(L.lib(), s)
    for s in ("fit_vae", "PlateauStopper", "VAEFitResult", "simple_vae_experiment", "write_clustering_metrics"):
        assert s in hlmc_amd.__all__ and hasattr(hlmc_amd, s)
    assert hlmc_amd.results.write_clustering_metrics is hlmc_amd.write_clustering_metrics
    assert hlmc_amd.baselines.simple_vae_experiment is hlmc_amd.simple_vae_experiment


# ------------------------------------------------------------------------------------------------ the table
ROWS = [{"Method": "VAE + KMeans", "Silhouette": 0.25, "Calinski-Harabasz": 120.5, "Architecture": "Simple VAE"},
        {"Method": "PCA + KMeans", "Silhouette": 0.125, "Calinski-Harabasz": 80.0, "Architecture": "Simple VAE"}]


def test_write_clustering_metrics_creates_the_file(tmp_path):
    import pandas as pd
    path = hlmc_amd.write_clustering_metrics(str(tmp_path / "results"), ROWS, "Simple VAE")
    assert path == os.path.join(str(tmp_path / "results"), "clustering_metrics.csv")
    df = pd.read_csv(path)
    assert list(df.columns) == ["Method", "Silhouette", "Calinski-Harabasz", "Architecture"]   # no index column
    assert df.to_dict("records") == ROWS


def test_write_clustering_metrics_replaces_only_its_own_rows(tmp_path):
    import pandas as pd
    d = str(tmp_path)
    other = pd.DataFrame({"Method": ["CVAE + KMeans", "Autoencoder + K-Means"], "Silhouette": [0.5, 0.4],
                          "Calinski-Harabasz": [10.0, 9.0], "NMI": [0.3, 0.2], "ARI": [0.1, 0.05],
                          "Purity": [0.6, 0.5], "Architecture": "Conditional VAE"})
    stale = pd.DataFrame([{**ROWS[0], "Silhouette": -1.0}])
    pd.concat([stale, other], ignore_index=True).to_csv(os.path.join(d, "clustering_metrics.csv"), index=False)
    hlmc_amd.write_clustering_metrics(d, ROWS, "Simple VAE")
    df = pd.read_csv(os.path.join(d, "clustering_metrics.csv"))
    assert list(df["Architecture"]) == ["Conditional VAE"] * 2 + ["Simple VAE"] * 2     # the others first, then ours
    assert list(df["Silhouette"]) == [0.5, 0.4, 0.25, 0.125]                            # the stale row is gone
    assert set(df.columns) == {"Method", "Silhouette", "Calinski-Harabasz", "NMI", "ARI", "Purity", "Architecture"}
    assert list(df["NMI"][:2]) == [0.3, 0.2] and df["NMI"][2:].isna().all()            # their columns kept, ours empty
    hlmc_amd.write_clustering_metrics(d, ROWS, "Simple VAE")                            # again: no duplicates
    assert len(pd.read_csv(os.path.join(d, "clustering_metrics.csv"))) == 4
    # the architecture argument names the rows, whatever the records say
    hlmc_amd.write_clustering_metrics(d, [{"Method": "m", "Silhouette": 0.0, "Calinski-Harabasz": 1.0}], "Conv VAE")
    df = pd.read_csv(os.path.join(d, "clustering_metrics.csv"))
    assert list(df["Architecture"]).count("Conv VAE") == 1 and len(df) == 5


@pytest.mark.parametrize("content", [b"", b"\xff\xfe\x00garbage\x00\x01", b"a,b\n1,2\n"])
def test_write_clustering_metrics_survives_an_unreadable_file(tmp_path, content):
    """An empty file, bytes that are no text, and a table without an 'Architecture' column: a fresh file, as the
    reference's except branch leaves."""
    import pandas as pd
    p = tmp_path / "clustering_metrics.csv"
    p.write_bytes(content)
    hlmc_amd.write_clustering_metrics(str(tmp_path), ROWS, "Simple VAE")
    assert pd.read_csv(p).to_dict("records") == ROWS


def test_write_clustering_metrics_refuses_no_rows(tmp_path):
    with pytest.raises(ValueError):
        hlmc_amd.write_clustering_metrics(str(tmp_path), [], "Simple VAE")
