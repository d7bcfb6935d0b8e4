"""fit_conv_vae (the training runs of src/Convolutional_VAE.py:202-303 and src/Conditional_VAE.py:310-402, and their
tables), the parts that need no GPU: the split against live torch, the host restatement of hlmc_fit_epoch_totals, the
host-side argument checks of the new entry point, fit_conv_vae's own argument errors and the two scripts' row builders."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from hlmc_amd import baselines as BL
from tests import conv_fit_cases as CC

ONE = C.c_void_p(256)          # non-null placeholder: validation fails before anything is dereferenced
NULL = None
U = 2.0 ** -53


def _err():
    return L.lib().hlmc_last_error().decode()


# ------------------------------------------------------------------------------------------------ random_split_indices
@pytest.mark.parametrize("n", [2, 23, 80, 1336])
@pytest.mark.parametrize("explicit", [True, False], ids=["explicit generator", "global generator"])
def test_random_split_indices_equal_live_torch(n, explicit):
    train = int(0.85 * n)
    lengths = [train, n - train]
    assert int((1 - 0.15) * n) == train                       # fit_conv_vae's default val_fraction is the script's 0.85
    assert hlmc_amd.train.split_sizes(n) == (train, n - train) and hlmc_amd.train.split_sizes(n, 0.0) == (n, 0)
    if explicit:
        ga, gb = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
        want = torch.utils.data.random_split(range(n), lengths, generator=ga)
        got = hlmc_amd.random_split_indices(n, lengths, generator=gb)
        assert torch.equal(ga.get_state(), gb.get_state())
    else:
        torch.manual_seed(11)
        want = torch.utils.data.random_split(range(n), lengths)
        state = torch.get_rng_state()
        torch.manual_seed(11)
        got = hlmc_amd.random_split_indices(n, lengths)
        assert torch.equal(torch.get_rng_state(), state)
    assert len(got) == 2
    for w, g in zip(want, got):
        assert g.dtype == torch.int64 and g.tolist() == list(w.indices)
    assert sorted(got[0].tolist() + got[1].tolist()) == list(range(n))


def test_random_split_indices_takes_three_parts_and_refuses_bad_lengths():
    g = torch.Generator().manual_seed(3)
    want = torch.utils.data.random_split(range(10), [5, 3, 2], generator=torch.Generator().manual_seed(3))
    got = hlmc_amd.random_split_indices(10, [5, 3, 2], generator=g)
    assert [t.tolist() for t in got] == [list(w.indices) for w in want]
    state = torch.get_rng_state()
    for bad in ([5, 4], [5, 6], [0.5, 0.5], [8.0, 2.0], [11, -1], [True, 9], []):
        with pytest.raises(ValueError):
            hlmc_amd.random_split_indices(10, bad)
    assert torch.equal(torch.get_rng_state(), state)          # a refused call draws nothing


# ------------------------------------------------------------------------------------------------ the restatement
def _gamma(k):
    return k * U / (1.0 - k * U)


@pytest.mark.parametrize("nt,nv", [(1, 1), (3, 1), (9, 2), (37, 7)])
def test_epoch_totals_restatement_against_longdouble(nt, nv):
    """Rounding count of a total: text_weight s1, the inner add, beta kld and the outer add touch a row's value at most
    3 times per term, the accumulation adds rows - 1 roundings and the division one: gamma(rows + 3) times the sum of
    the terms' magnitudes.  The plain sums (audio, text, kld): rows - 1 additions and the division, gamma(rows)."""
    tw, beta, td, vd = 350.0, 1.0, 19.0, 4.0
    tr, va = CC.epoch_totals_cases(nt, nv)
    got = CC.epoch_totals(tr.tolist(), va.tolist(), tw, beta, td, vd)
    ld = np.longdouble

    def exact(t, div):
        t = t.astype(ld)
        terms = np.stack([t[:, 0], ld(tw) * t[:, 1], ld(beta) * ld(-0.5) * t[:, 2]], axis=1)
        return terms.sum() / ld(div), np.abs(terms).sum() / ld(div)

    want, mag = exact(tr, td)
    assert abs(ld(got[0]) - want) <= _gamma(nt + 3) * mag
    want, mag = exact(va, vd)
    assert abs(ld(got[4]) - want) <= _gamma(nv + 3) * mag
    for i, col in ((1, tr[:, 0]), (2, tr[:, 1]), (3, -0.5 * tr[:, 2])):
        c = col.astype(ld)
        assert abs(ld(got[i]) - c.sum() / ld(td)) <= _gamma(nt) * np.abs(c).sum() / ld(td)
    assert (tr[:, 2] < 0).any() and (nt == 1 or (tr[:, 2] > 0).any())


def test_epoch_totals_restatement_by_hand():
    tr = [(8.0, 0.5, -4.0), (2.0, 0.25, 2.0)]
    va = [(1.0, 1.0, -1.0)]
    # kld = 2, -1; totals (8 + 100) + 4 * 2 = 116 and (2 + 50) - 4 = 48
    assert CC.epoch_totals(tr, va, 200.0, 4.0, 2.0, 1.0) == (82.0, 5.0, 0.375, 0.5, (1.0 + 200.0) + 4.0 * 0.5)


# ------------------------------------------------------------------------------------------------ host checks
TOTALS_OK = dict(train=ONE, nt=3, val=ONE, nv=1, tw=350.0, beta=1.0, td=19.0, vd=4.0, out=ONE)
NAN = float("nan")


@pytest.mark.parametrize("bad", [dict(train=NULL), dict(val=NULL), dict(out=NULL), dict(nt=0), dict(nt=-1), dict(nv=0),
                                 dict(nv=-5), dict(td=0.0), dict(td=-1.0), dict(vd=0.0), dict(vd=-2.0), dict(tw=NAN),
                                 dict(beta=NAN), dict(td=NAN), dict(vd=NAN)])
def test_fit_epoch_totals_checks_its_arguments_on_the_host(bad):
    a = {**TOTALS_OK, **bad}
    st = L.lib().hlmc_fit_epoch_totals(None, a["train"], a["nt"], a["val"], a["nv"], a["tw"], a["beta"], a["td"],
                                       a["vd"], a["out"])
    assert st == -1 and "fit_epoch_totals" in _err()


def test_new_symbols_are_bound_and_exported():
    assert "hlmc_fit_epoch_totals" in L.exported_symbols() and hasattr(L.lib(), "hlmc_fit_epoch_totals")
    for s in ("random_split_indices", "fit_conv_vae", "ConvFitResult", "extract_latents",
              "convolutional_vae_experiment", "conditional_vae_experiment"):
        assert s in hlmc_amd.__all__ and hasattr(hlmc_amd, s)
    assert hlmc_amd.train.fit_conv_vae is hlmc_amd.fit_conv_vae
    assert hlmc_amd.baselines.convolutional_vae_experiment is hlmc_amd.convolutional_vae_experiment
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hlmc.h")) as f:
        assert "int hlmc_fit_epoch_totals(void* stream, const double* train_sums, int nt" in f.read()


# ------------------------------------------------------------------------------------------------ fit_conv_vae arguments
def test_fit_conv_vae_argument_errors_come_before_any_launch():
    """CPU models: an error that came after the first launch would be the engine's HLMCError instead."""
    fit = hlmc_amd.fit_conv_vae
    hyb, aud, cv = (CC.build(k, 1, device=None) for k in ("hybrid", "audio", "cvae"))
    a, t, _ = CC.make_data("hybrid", 23)
    a2, _, _ = CC.make_data("audio", 23)
    ac, tc, cc = CC.make_data("cvae", 23)
    others = (hlmc_amd.VAE(8, [8, 4], 3), hlmc_amd.SimpleAutoencoder(8, 3), torch.nn.Linear(8, 8))
    state = torch.get_rng_state()
    for wrong in others:
        with pytest.raises(TypeError):
            fit(wrong, a, t)
    with pytest.raises(ValueError, match="cond"):
        fit(cv, ac, tc)                                            # missing cond
    with pytest.raises(ValueError, match="text"):
        fit(cv, ac, cond=cc)
    with pytest.raises(ValueError, match="text"):
        fit(aud, a2, torch.zeros(23, 768))                         # text given to an audio-only model
    with pytest.raises(ValueError, match="text"):
        fit(hyb, a)
    with pytest.raises(ValueError, match="cond"):
        fit(hyb, a, t, cc)
    with pytest.raises(ValueError, match="rows"):
        fit(hyb, a, t[:22])                                        # row-count mismatch
    with pytest.raises(ValueError, match="rows"):
        fit(cv, ac, tc, cc[:5])
    with pytest.raises(ValueError):
        fit(hyb, a2, t)                                            # 64 x 128 images for a 64 x 64 model
    with pytest.raises(ValueError):
        fit(hyb, a, torch.zeros(23, 384))
    with pytest.raises(ValueError):
        fit(cv, ac, tc, torch.zeros(23, 9))
    with pytest.raises(ValueError, match="one row"):
        fit(hyb, a[:21], t[:21], batch_size=4)                     # 17 training rows: a tail of 1
    with pytest.raises(ValueError, match="one row"):
        fit(hyb, a, t, batch_size=1)
    with pytest.raises(ValueError, match="one row"):
        fit(hyb, a, t, batch_size=8, split=(torch.arange(9), torch.arange(9, 23)))
    with pytest.raises(ValueError, match="validation"):
        fit(hyb, a[:1], t[:1])                                     # int(0.85 * 1) = 0 training rows
    with pytest.raises(ValueError, match="validation"):
        fit(hyb, a, t, val_fraction=0.0)                           # no validation rows
    with pytest.raises(ValueError, match="validation"):
        fit(hyb, a, t, split=(torch.arange(23), torch.arange(0)))
    with pytest.raises(ValueError, match="outside"):
        fit(hyb, a, t, split=(torch.arange(20), torch.arange(20, 24)))
    for bad in (float("nan"), float("inf")):
        x = a.clone()
        x[22, 0, 63, 63] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            fit(hyb, x, t)                                         # a non-finite input
        y = tc.clone()
        y[0, 0] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            fit(cv, ac, y, cc)
    for kw in (dict(epochs=0), dict(batch_size=0), dict(patience=0), dict(normalize="rows")):
        with pytest.raises(ValueError):
            fit(hyb, a, t, **kw)
    assert torch.equal(torch.get_rng_state(), state)               # no refused call drew a split
    with pytest.raises(L.HLMCError):                               # a CPU model: refused, never computed in eager torch
        fit(hyb, a, t, epochs=1, batch_size=8)
    with pytest.raises(L.HLMCError):
        hlmc_amd.extract_latents(hyb, a, t)
    with pytest.raises(ValueError):
        hlmc_amd.extract_latents(hyb, a, t[:3])


def test_fit_conv_vae_defaults_are_the_two_scripts():
    import inspect
    p = inspect.signature(hlmc_amd.fit_conv_vae).parameters
    assert [p[k].default for k in ("epochs", "batch_size", "lr", "val_fraction", "restore_best")] == [500, 32, 1e-4, 0.15,
                                                                                                     False]
    assert all(p[k].default is None for k in ("beta", "text_weight", "patience", "normalize", "generator", "split"))
    from hlmc_amd.train import _CONV_DEFAULTS
    assert _CONV_DEFAULTS == {"hybrid": dict(beta=1.0, text_weight=350.0, patience=15, normalize="samples"),
                              "cvae": dict(beta=4.0, text_weight=200.0, patience=20, normalize="batches")}


# ------------------------------------------------------------------------------------------------ the rows
def _conv_rows(labels=None):
    rec = CC.RECORDED_CONV
    names = BL.conv_vae_algorithm_names(*rec["best"])
    return [BL.conv_vae_row(n, l, s) for n, l, s in zip(names, labels or rec["labels"], rec["scores"])]


def test_convolutional_rows_are_the_scripts():
    assert BL.conv_vae_algorithm_names(5, 3, 7.0) == ["K-Means-Main (k=5)", "K-Means-Language (k=2)",
                                                      "Agglomerative (k=3)", "DBSCAN (eps=7.0)"]
    assert BL.conv_vae_algorithm_names(2, 14, np.float64(10.0))[3] == "DBSCAN (eps=10.0)"
    rows = _conv_rows()
    for r in rows:
        assert list(r) == ["Algorithm", "Silhouette", "Davies-Bouldin", "ARI", "n_clusters", "Architecture"]
        assert r["Architecture"] == "Convolutional VAE"
    assert [r["n_clusters"] for r in rows] == [5, 2, 3, 1]          # noise is no cluster
    assert rows[0]["Silhouette"] == 0.25 and rows[0]["Davies-Bouldin"] == 1.5 and rows[0]["ARI"] == 0.125
    assert rows[2]["ARI"] is None                                   # no ground truth
    # one cluster plus noise: the script's -1 row, the scores never asked for
    assert (rows[3]["Silhouette"], rows[3]["Davies-Bouldin"], rows[3]["ARI"]) == (-1, -1, -1)

    def never():
        raise AssertionError("scores of a single-cluster labelling were computed")
    single = BL.conv_vae_row("DBSCAN (eps=3.0)", np.zeros(9, dtype=np.int64), never)
    assert single["n_clusters"] == 1 and single["Silhouette"] == -1
    noise = BL.conv_vae_row("DBSCAN (eps=3.0)", -np.ones(9, dtype=np.int64), never)
    assert noise["n_clusters"] == 0 and noise["ARI"] == -1
    assert BL.conv_vae_row("x", [0, 1, -1], lambda: CC.RECORDED_CONV["scores"][0])["n_clusters"] == 2


def test_conditional_rows_are_the_scripts():
    rows = [BL.cvae_row(m, s) for m, s in CC.RECORDED_CVAE]
    assert [r["Method"] for r in rows] == ["CVAE (Multi-Modal)", "PCA + K-Means", "Autoencoder + K-Means",
                                           "Direct Spectral"]
    for r, (_, s) in zip(rows, CC.RECORDED_CVAE):
        assert list(r) == ["Silhouette", "NMI", "ARI", "Purity", "Method", "Architecture"]
        assert r["Architecture"] == "Conditional VAE"
        assert all(r[k] == s[k] for k in ("Silhouette", "NMI", "ARI", "Purity"))


SIMPLE = [{"Method": "VAE + KMeans", "Silhouette": 0.25, "Calinski-Harabasz": 120.5, "Architecture": "Simple VAE"},
          {"Method": "PCA + KMeans", "Silhouette": 0.125, "Calinski-Harabasz": 80.0, "Architecture": "Simple VAE"}]


def test_rows_merge_into_a_table_that_holds_simple_vae_rows(tmp_path):
    import pandas as pd
    d = str(tmp_path)
    path = hlmc_amd.write_clustering_metrics(d, SIMPLE, "Simple VAE")
    hlmc_amd.write_clustering_metrics(d, _conv_rows(), "Convolutional VAE")
    hlmc_amd.write_clustering_metrics(d, [BL.cvae_row(m, s) for m, s in CC.RECORDED_CVAE], "Conditional VAE")
    hlmc_amd.write_clustering_metrics(d, _conv_rows(), "Convolutional VAE")      # again: replaced, not duplicated
    df = pd.read_csv(path)
    assert list(df["Architecture"]) == ["Simple VAE"] * 2 + ["Conditional VAE"] * 4 + ["Convolutional VAE"] * 4
    simple = df[df["Architecture"] == "Simple VAE"]
    assert simple[["Method", "Silhouette", "Calinski-Harabasz", "Architecture"]].to_dict("records") == SIMPLE
    assert simple["Algorithm"].isna().all() and simple["NMI"].isna().all()
    conv = df[df["Architecture"] == "Convolutional VAE"]
    assert list(conv["Algorithm"]) == BL.conv_vae_algorithm_names(*CC.RECORDED_CONV["best"])
    assert list(conv["n_clusters"]) == [5, 2, 3, 1] and list(conv["Silhouette"]) == [0.25, 0.5, 0.375, -1.0]
    assert np.isnan(conv["ARI"].iloc[2]) and conv["ARI"].iloc[3] == -1.0
    cvae = df[df["Architecture"] == "Conditional VAE"]
    assert list(cvae["Purity"]) == [0.75, 0.5, 0.625, 0.375] and cvae["Calinski-Harabasz"].isna().all()
