"""hlmc_silhouette_batch (csrc/metrics.hip) through hlmc_amd._lib as include/hlmc.h declares it, and the Python surface
on top of it: metrics.silhouette_scores, cluster.kmeans_k_sweep and the two sweeps that moved onto the batched call.

The contract needs no tolerance: for every labelling m of a batch, S[:, off_m : off_m + ks[m]], its counts, samples and
score have the same BYTES as one hlmc_silhouette call on that labelling alone.  Independently, each lies within
oracle/metrics_oracle.py's bounds (sums_bound / samples_bound / score_bound, derived from the number formats) of the
float64 direct-difference reference.  Outputs and the workspace are pre-filled with NaN, each output has one spare
element, and S and the counts are read back through the documented layout: nothing is left unwritten, nothing is
written past an end, samples == NULL writes no sample, a second call is bit-identical.

Shapes: tests/silhouette_batch_cases.py.  Every case prints its worst |err| / bound as "RATIO <quantity> <case> <value>"."""
import functools

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import metrics_oracle as MT
from tests import metrics_cases as MC
from tests import silhouette_batch_cases as BC

pytestmark = pytest.mark.gpu
M = hlmc_amd.metrics
PART = 512          # block partials per labelling (kSilFinalBlocks)


def _nan64(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _r256(b):
    return (b + 255) // 256 * 256


def _ratio(err, bound):
    err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    assert (err[bound == 0] == 0).all(), "non-zero error where the reference is exact"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _ks_array(ks):
    return (L.C.c_int32 * len(ks))(*ks)


def _batch(Xd, labd, ks, want_samples):
    """One hlmc_silhouette_batch call on NaN-filled buffers -> (S [n][K], counts [K], samples [M][n] or None, scores [M])."""
    n, d = Xd.shape
    m, K = len(ks), int(sum(ks))
    lib = L.lib()
    nbytes = int(lib.hlmc_silhouette_batch_workspace(n, _ks_array(ks), m))
    assert nbytes == _r256(n * K * 8) + _r256(4 * K) + m * PART * 8          # the documented layout
    ws = _nan64(nbytes // 8 + 1)                                              # one spare element behind the workspace
    samples = _nan64(m * n + 1)
    scores = _nan64(m + 1)
    L.check(lib.hlmc_silhouette_batch(L.stream(), Xd.data_ptr(), n, d, labd.data_ptr(), _ks_array(ks), m,
                                      samples.data_ptr() if want_samples else None, scores.data_ptr(), ws.data_ptr(),
                                      nbytes), "hlmc_silhouette_batch")
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    assert np.isnan(w[-1]), "wrote past the workspace"
    off = _r256(n * K * 8)
    S = w[:n * K].reshape(n, K).copy()
    counts = w.view(np.int32)[off // 4: off // 4 + K].copy()
    sc = scores.cpu().numpy()
    assert np.isnan(sc[m]), "scores wrote past its end"
    smp = samples.cpu().numpy()
    if want_samples:
        assert np.isnan(smp[m * n]), "samples wrote past its end"
    else:
        assert np.isnan(smp).all(), "samples == NULL but something was written"
    return S, counts, (smp[:m * n].reshape(m, n) if want_samples else None), sc[:m].copy()


def _single(Xd, labd, k):
    """One hlmc_silhouette call on NaN-filled buffers -> (S [n][k], counts [k], samples [n], score)."""
    n, d = Xd.shape
    lib = L.lib()
    nbytes = int(lib.hlmc_silhouette_workspace(n, k))
    ws, samples, score = _nan64(nbytes // 8), _nan64(n), _nan64(1)
    L.check(lib.hlmc_silhouette(L.stream(), Xd.data_ptr(), n, d, labd.data_ptr(), k, samples.data_ptr(),
                                score.data_ptr(), ws.data_ptr(), nbytes), "hlmc_silhouette")
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    off = _r256(n * k * 8)
    return (w[:n * k].reshape(n, k).copy(), w.view(np.int32)[off // 4: off // 4 + k].copy(), samples.cpu().numpy(),
            score.cpu().numpy()[0])


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The case's inputs and, per labelling, the float64 oracle's (S, samples): computed once, read-only."""
    X, Y, ks = BC.case_input(BC.CASES[BC.IDS.index(name)])
    refs = []
    for y in Y:
        S = MT.silhouette_sums(X, y)
        s = MT.silhouette_from_sums(S, y)
        S.setflags(write=False)
        s.setflags(write=False)
        refs.append((S, s))
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, ks, refs


def test_cases_hold_what_they_are_for():
    """The k sweep has more columns than one window and a labelling that straddles a window boundary, at both
    window widths include/hlmc.h documents; the wide labelling spans more than a whole window; the M = 40 / 64 cases
    put more labellings into one window than the sweep does."""
    for d in (16, 128):
        kw = BC.kw_max(d)
        assert sum(BC.SWEEP_KS) == 104 > kw
        assert BC.straddlers(BC.SWEEP_KS, kw) == [9]           # k = 11 at [54, 65) crosses 58 and 64
    assert BC.offsets(BC.SWEEP_KS)[9] == 54
    assert 129 > 2 * BC.kw_max(16) and BC.straddlers((3, 129), BC.kw_max(16)) == [1]
    assert BC.kw_max(33) // 2 > len(BC.SWEEP_KS) and BC.MAX_BATCH * 2 > BC.kw_max(33)


@pytest.mark.parametrize("name", BC.IDS)
def test_batch_equals_single_calls_bit_for_bit_and_sits_inside_the_oracle_bounds(cuda, name):
    X, Y, ks, refs = _reference(name)
    n, d = X.shape
    Xd = torch.as_tensor(np.array(X), device="cuda")
    labd = torch.as_tensor(np.array(Y), device="cuda")
    S, counts, samples, scores = _batch(Xd, labd, ks, True)
    assert not np.isnan(S).any(), "S has unwritten elements"
    assert not np.isnan(samples).any() and not np.isnan(scores).any(), "samples / scores have unwritten elements"
    off = BC.offsets(ks)
    worst = dict(S=0.0, samples=0.0, score=0.0)
    for m, k in enumerate(ks):
        a, b = int(off[m]), int(off[m + 1])
        S1, c1, s1, sc1 = _single(Xd, labd[m].contiguous(), k)
        assert S[:, a:b].tobytes() == S1.tobytes(), f"labelling {m}: S differs from the single call"
        assert counts[a:b].tobytes() == c1.tobytes(), f"labelling {m}: counts differ from the single call"
        assert samples[m].tobytes() == s1.tobytes(), f"labelling {m}: samples differ from the single call"
        assert scores[m].tobytes() == sc1.tobytes(), f"labelling {m}: score differs from the single call"
        np.testing.assert_array_equal(counts[a:b], np.bincount(Y[m], minlength=k))
        S_ref, s_ref = refs[m]
        worst["S"] = max(worst["S"], _ratio(np.abs(S[:, a:b] - S_ref), MT.sums_bound(S_ref, d)))
        worst["samples"] = max(worst["samples"], _ratio(np.abs(samples[m] - s_ref), MT.samples_bound(s_ref, d)))
        worst["score"] = max(worst["score"], abs(scores[m] - float(np.mean(s_ref))) / MT.score_bound(s_ref, d))
    print("\n".join(f"RATIO {q} {name} {v:.4f}" for q, v in worst.items()))
    for q, v in worst.items():
        assert v <= 1.0, f"{q} outside its derived bound: {v}"
    if name == "same_three_times":
        assert S[:, 0:5].tobytes() == S[:, 5:10].tobytes() == S[:, 10:15].tobytes()
        assert samples[0].tobytes() == samples[1].tobytes() == samples[2].tobytes()
        assert scores[0].tobytes() == scores[1].tobytes() == scores[2].tobytes()
    S0, c0, none, scores0 = _batch(Xd, labd, ks, False)
    assert none is None and scores0.tobytes() == scores.tobytes(), "samples == NULL changes the scores"
    S2, c2, samples2, scores2 = _batch(Xd, labd, ks, True)
    assert S2.tobytes() == S.tobytes() == S0.tobytes() and samples2.tobytes() == samples.tobytes()
    assert scores2.tobytes() == scores.tobytes() and c2.tobytes() == counts.tobytes() == c0.tobytes()


# ---------------------------------------------------------------- metrics.silhouette_scores
def _wrapper_labelings():
    sem = MC.sil_semantic_inputs()
    X = sem["dbscan_noise_label"][0]
    rng = np.random.default_rng(11)
    return X, [sem["dbscan_noise_label"][1], sem["string_labels"][1], sem["singleton"][1],
               rng.integers(0, 70, 203).astype(np.int64), torch.as_tensor(rng.integers(3, 7, 203))]


def test_silhouette_scores_equals_silhouette_score_per_labelling(cuda):
    """Labellings with DBSCAN's -1, strings, a singleton, 70 labels (more than one window) and a tensor: every score
    has the bytes of silhouette_score on that labelling, whatever the chunking, and return_samples gives
    silhouette_samples per labelling."""
    X, labelings = _wrapper_labelings()
    assert (labelings[0] == -1).any() and labelings[1].dtype.kind == "U"
    want = np.array([M.silhouette_score(X, y) for y in labelings])
    got = M.silhouette_scores(X, labelings)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (len(labelings),)
    assert got.tobytes() == want.tobytes()
    Xd = torch.as_tensor(X, device="cuda")
    one_each = M.silhouette_scores(Xd, labelings, workspace_cap=1)          # every labelling its own chunk
    mixed = M.silhouette_scores(Xd, labelings, workspace_cap=203 * 8 * 12)
    assert one_each.tobytes() == want.tobytes() and mixed.tobytes() == want.tobytes()
    for cap in (None, 1):
        scores, samples = M.silhouette_scores(Xd, labelings, return_samples=True, workspace_cap=cap)
        assert scores.tobytes() == want.tobytes()
        assert samples.is_cuda and samples.dtype == torch.float64 and samples.shape == (len(labelings), 203)
        for m, y in enumerate(labelings):
            assert samples[m].cpu().numpy().tobytes() == M.silhouette_samples(Xd, y).cpu().numpy().tobytes(), m


def test_silhouette_scores_more_labellings_than_one_call_holds(cuda):
    """70 labellings: two hlmc_silhouette_batch calls (64 + 6) behind one silhouette_scores call."""
    X = MC.normals(90, 8, seed=3)
    labelings = [MC.labels(90, 2 + m % 3, seed=m) for m in range(BC.MAX_BATCH + 6)]
    want = np.array([M.silhouette_score(X, y) for y in labelings])
    assert M.silhouette_scores(X, labelings).tobytes() == want.tobytes()


def test_silhouette_scores_names_the_bad_labelling(cuda):
    X = MC.normals(20, 4, seed=1)
    good = MC.labels(20, 3, seed=1)
    with pytest.raises(ValueError, match=r"labelling 1: Number of labels is 1\. Valid values are 2 to n_samples - 1"):
        M.silhouette_scores(X, [good, np.zeros(20, dtype=np.int64)])
    with pytest.raises(ValueError, match=r"labelling 2: Number of labels is 20\."):
        M.silhouette_scores(X, [good, good, np.arange(20)])
    with pytest.raises(ValueError, match="labelling 0 has 19 entries"):
        M.silhouette_scores(X, [good[:19]])
    with pytest.raises(ValueError, match="euclidean"):
        M.silhouette_scores(X, [good], metric="cosine")
    assert M.silhouette_scores(X, []).shape == (0,)


# ---------------------------------------------------------------- the three sweeps
def test_kmeans_k_sweep_matches_single_fits_sklearn_and_the_reference_rule(cuda):
    from sklearn.cluster import KMeans as SkKMeans
    X = BC.blobs(300, 8, 4, seed=5)
    k_range = range(2, 7)
    best, records = hlmc_amd.kmeans_k_sweep(X, k_range, n_init=3)
    assert [r["k"] for r in records] == list(k_range)
    want_best, want_sil = 2, -1          # src/Convolutional_VAE.py:311-329
    for k, rec in zip(k_range, records):
        km = hlmc_amd.KMeans(n_clusters=k, random_state=42, n_init=3).fit(X)
        assert rec["labels"].dtype == km.labels_.dtype and rec["labels"].tobytes() == km.labels_.tobytes(), k
        assert rec["inertia"] == km.inertia_, k
        assert np.array_equal(rec["labels"], SkKMeans(n_clusters=k, random_state=42, n_init=3).fit_predict(X)), k
        sil = M.silhouette_score(X, rec["labels"])
        assert isinstance(rec["silhouette"], float) and rec["silhouette"] == sil, k
        if sil > want_sil:
            want_best, want_sil = k, sil
    assert best == want_best
    again = hlmc_amd.kmeans_k_sweep(torch.as_tensor(X, device="cuda"), k_range, n_init=3)
    assert again[0] == best
    for ra, rb in zip(records, again[1]):
        assert ra["labels"].tobytes() == rb["labels"].tobytes()
        assert ra["inertia"] == rb["inertia"] and ra["silhouette"] == rb["silhouette"]
    with pytest.raises(ValueError, match="every k must be in"):
        hlmc_amd.kmeans_k_sweep(X, [2, 300])


def test_agglomerative_k_sweep_silhouettes_are_the_single_scores(cuda):
    from tests import ward_check as WK
    X = WK.case_input("latents")
    best, records = hlmc_amd.agglomerative_k_sweep(X)
    assert [r["k"] for r in records] == list(WK.K_RANGE)
    for rec in records:
        assert isinstance(rec["silhouette"], float)
        assert np.float64(rec["silhouette"]).tobytes() == np.float64(M.silhouette_score(X, rec["labels"])).tobytes()


@pytest.mark.parametrize("cap", [None, 1])
def test_dbscan_eps_sweep_silhouettes_are_the_single_scores(cuda, cap):
    from tests import dbscan_check as DK
    X = DK.case_input("blobs_n1000_d32")
    best, records = hlmc_amd.dbscan_eps_sweep(X, np.arange(4.0, 13.0, 1.0), min_samples=5, workspace_cap=cap)
    scored = 0
    for rec in records:
        if rec["n_clusters"] >= 2:
            assert isinstance(rec["silhouette"], float)
            assert np.float64(rec["silhouette"]).tobytes() == np.float64(M.silhouette_score(X, rec["labels"])).tobytes()
            scored += 1
        else:
            assert rec["silhouette"] is None
    assert scored >= 2
    if cap is None:          # all noise, all noise, one cluster: nothing is passed down, every record keeps None
        best, records = hlmc_amd.dbscan_eps_sweep(DK.case_input("blobs_n777_d16"), [0.05, 0.1, 500.0])
        assert best == 10.0 and [r["silhouette"] for r in records] == [None, None, None]
