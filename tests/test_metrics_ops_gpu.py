"""Op-level parity of the cluster-quality kernels (csrc/metrics.hip), called through hlmc_amd._lib as
include/hlmc.h declares them, against oracle/metrics_oracle.py: float64 direct-difference silhouette sums and
longdouble centroid / dispersion statistics, each with a bound derived from the roundings the kernel's number formats
allow (never from a kernel's output; tests/test_oracle_cpu.py holds a float32 restatement of the kernel inside the
same bounds on the same inputs).  Shapes sit on the edges the code has: the DMAX 32 / 64 / 128 dispatch, the zero-padded
float4 tail, the 64-row block and tile, the label windows of 64 (DMAX 32 / 64) and 62 (DMAX 128) accumulator rows,
k = n - 1, the 256-thread column loop and the 3-label LDS window at d = 4096, 64 KiB of LDS at k = 1024.

Outputs and the workspace are pre-filled with NaN and the workspace is read back (layouts: include/hlmc.h), so an
element left unwritten shows as NaN.  Labels are always in [0, k) with every label present: the kernels index with
them unchecked (include/hlmc.h states the precondition).

Every test prints its worst |err| / bound as "RATIO <quantity> <case> <value>"."""
import functools

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import metrics_oracle as MT
from tests import metrics_cases as MC

pytestmark = pytest.mark.gpu
M = hlmc_amd.metrics
KCLU = 64          # row blocks of the cluster-score kernels (kCluBlocks)


def _nan64(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _ratio(err, bound):
    """max err / bound; an element with bound 0 must have err 0 (and counts as ratio 0)."""
    err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    assert (err[bound == 0] == 0).all(), "non-zero error where the reference is exact"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _silhouette(Xd, labd, k, want_samples):
    """One hlmc_silhouette call on NaN-filled buffers -> (S [n][k], counts [k], samples [n + 1] or None, score)."""
    n, d = Xd.shape
    lib = L.lib()
    nbytes = int(lib.hlmc_silhouette_workspace(n, k))
    assert nbytes % 8 == 0
    ws = _nan64(nbytes // 8)
    samples = _nan64(n + 1)                 # one spare element: a write past the end shows
    score = _nan64(2)
    L.check(lib.hlmc_silhouette(L.stream(), Xd.data_ptr(), n, d, labd.data_ptr(), k,
                                samples.data_ptr() if want_samples else None, score.data_ptr(), ws.data_ptr(), nbytes),
            "hlmc_silhouette")
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    off = (n * k * 8 + 255) // 256 * 256    # counts: the next 256-byte boundary after S
    S = w[:n * k].reshape(n, k).copy()
    counts = w.view(np.int32)[off // 4: off // 4 + k].copy()
    sc = score.cpu().numpy()
    assert np.isnan(sc[1]), "score wrote past its scalar"
    smp = samples.cpu().numpy()
    if want_samples:
        assert np.isnan(smp[n]), "samples wrote past its end"
    else:
        assert np.isnan(smp).all(), "samples == NULL but something was written"
    return S, counts, (smp[:n] if want_samples else None), float(sc[0])


@functools.lru_cache(maxsize=None)
def _sil_reference(name):
    case = MC.SIL_CASES[MC.SIL_IDS.index(name)]
    X, y, k = MC.sil_input(case)
    S = MT.silhouette_sums(X, y)
    s = MT.silhouette_from_sums(S, y)
    for a in (X, y, S, s):
        a.setflags(write=False)
    return X, y, k, S, s


def _check_silhouette(name, X, y, k, S_ref, s_ref):
    n, d = X.shape
    Xd = torch.as_tensor(np.array(X), device="cuda")
    labd = torch.as_tensor(np.array(y, dtype=np.int32), device="cuda")
    S, counts, samples, score = _silhouette(Xd, labd, k, True)
    assert not np.isnan(S).any(), "S has unwritten elements"
    assert not np.isnan(samples).any(), "samples has unwritten elements"
    np.testing.assert_array_equal(counts, np.bincount(y, minlength=k))
    rS = _ratio(np.abs(S - S_ref), MT.sums_bound(S_ref, d))
    rs = _ratio(np.abs(samples - s_ref), MT.samples_bound(s_ref, d))
    rm = abs(score - float(np.mean(s_ref))) / MT.score_bound(s_ref, d)
    print(f"RATIO S {name} {rS:.4f}\nRATIO samples {name} {rs:.4f}\nRATIO score {name} {rm:.4f}")
    assert rS <= 1.0, f"S outside sums_bound: {rS}"
    assert rs <= 1.0, f"samples outside samples_bound: {rs}"
    assert rm <= 1.0, f"score outside the mean bound: {rm}"
    S0, c0, none, score0 = _silhouette(Xd, labd, k, False)
    assert none is None and np.float64(score0).tobytes() == np.float64(score).tobytes(), "samples == NULL changes the score"
    S2, c2, samples2, score2 = _silhouette(Xd, labd, k, True)
    assert S2.tobytes() == S.tobytes() == S0.tobytes() and samples2.tobytes() == samples.tobytes()
    assert np.float64(score2).tobytes() == np.float64(score).tobytes() and (c2 == counts).all() and (c0 == counts).all()
    return samples, score


@pytest.mark.parametrize("name", MC.SIL_IDS)
def test_silhouette_kernels_within_derived_bounds(cuda, name):
    """S (read back from the workspace), the per-sample coefficients and the score within sums_bound / samples_bound /
    their mean of the float64 direct-difference oracle; counts equal to bincount; nothing left unwritten; the score the
    same bits with and without samples; a second call bit-identical."""
    X, y, k, S_ref, s_ref = _sil_reference(name)
    _check_silhouette(name, X, y, k, S_ref, s_ref)


@pytest.mark.parametrize("name", list(MC.sil_semantic_inputs()))
def test_silhouette_sklearn_semantics(cuda, name):
    """sklearn's special cases through the Python wrappers (label encoding included), against live sklearn at the
    tolerances of tests/test_metrics_gpu.py and against the oracle within its bounds: a singleton scores 0, a cluster
    of exact duplicates scores 1 (a = 0), a = b = 0 scores 0, DBSCAN's -1 and strings are labels like any other."""
    from sklearn.metrics import silhouette_samples as sk_samples, silhouette_score as sk_score
    X, y = MC.sil_semantic_inputs()[name]
    enc = np.unique(y, return_inverse=True)[1].astype(np.int32)
    k = int(enc.max()) + 1
    S_ref = MT.silhouette_sums(X, enc)
    s_ref = MT.silhouette_from_sums(S_ref, enc)
    samples, score = _check_silhouette(name, X, enc, k, S_ref, s_ref)
    got = M.silhouette_samples(X, y).cpu().numpy()
    assert got.tobytes() == samples.tobytes(), "the wrapper's label encoding differs from np.unique's"
    assert np.float64(M.silhouette_score(torch.as_tensor(X, device="cuda"), y)).tobytes() == np.float64(score).tobytes()
    np.testing.assert_allclose(got, sk_samples(X, y), rtol=1e-5, atol=1e-6)
    ref = float(sk_score(X, y))
    assert abs(score - ref) <= 1e-6 * abs(ref) + 1e-8
    if name == "singleton":
        assert got[17] == 0.0
    elif name == "duplicates":
        assert (got[enc == 0] == 1.0).all()
    elif name == "identical_rows_in_two_clusters":
        assert (got[enc < 2] == 0.0).all() and (got[enc == 2] != 0.0).all()


def test_silhouette_score_sample_size(cuda):
    """silhouette_score(sample_size=97, random_state=3) at n = 400: sklearn's subset (RandomState(3).permutation(n)[:97])
    for numpy X, a device tensor X and tensor labels -- the same bits as scoring that subset directly, and live
    sklearn's value at the tolerance of tests/test_metrics_gpu.py."""
    from sklearn.metrics import silhouette_score as sk_score
    X = MC.normals(400, 10, seed=31)
    X[:200] += np.float32(1.5)
    y = MC.labels(400, 4, seed=31).astype(np.int64)
    y[:200] = np.minimum(y[:200], 1)
    idx = np.random.RandomState(3).permutation(400)[:97]
    direct = M.silhouette_score(X[idx], y[idx])
    ref = float(sk_score(X, y, sample_size=97, random_state=3))
    assert abs(direct - ref) <= 1e-6 * abs(ref) + 1e-8, (direct, ref)
    Xd = torch.as_tensor(X, device="cuda")
    for xx, yy in ((X, y), (Xd, y), (Xd, torch.as_tensor(y)), (X, torch.as_tensor(y, device="cuda"))):
        assert M.silhouette_score(xx, yy, sample_size=97, random_state=3) == direct
    assert M.silhouette_score(Xd, y, sample_size=97, random_state=np.random.RandomState(3)) == direct
    assert M.silhouette_score(X, y, sample_size=97, random_state=4) != direct


# ---------------------------------------------------------------- Davies-Bouldin / Calinski-Harabasz
def _cluster_scores(Xd, labd, k):
    """One hlmc_cluster_scores call on NaN-filled buffers -> dict(cent, mean, counts, intra, db, ch)."""
    n, d = Xd.shape
    lib = L.lib()
    nbytes = int(lib.hlmc_cluster_scores_workspace(k, d))
    assert nbytes % 8 == 0
    ws = _nan64(nbytes // 8)
    out = _nan64(3)
    L.check(lib.hlmc_cluster_scores(L.stream(), Xd.data_ptr(), n, d, labd.data_ptr(), k, out.data_ptr(), ws.data_ptr(),
                                    nbytes), "hlmc_cluster_scores")
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    o = KCLU * k * d + KCLU * k * 2                      # part | part2 | cent[k][d] | mean[d] | counts | intra[k]
    cent = w[o:o + k * d].reshape(k, d).copy()
    mean = w[o + k * d:o + k * d + d].copy()
    c_off = o + k * d + d
    counts = w.view(np.int32)[2 * c_off:2 * c_off + k].copy()
    i_off = c_off + (4 * k + 255) // 256 * 32
    assert i_off + k == nbytes // 8
    intra = w[i_off:i_off + k].copy()
    res = out.cpu().numpy()
    assert np.isnan(res[2]), "out2 wrote past its two scores"
    assert not np.isnan(w[:o]).any(), "block partials left unwritten"
    return dict(cent=cent, mean=mean, counts=counts, intra=intra, db=float(res[0]), ch=float(res[1]))


@functools.lru_cache(maxsize=None)
def _clu_reference(name):
    X, y, k = MC.clu_input(MC.CLU_CASES[MC.CLU_IDS.index(name)])
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y, k, MT.cluster_stats(X, y)


def _check_cluster_scores(name, X, y, k, st):
    Xd = torch.as_tensor(np.array(X), device="cuda")
    labd = torch.as_tensor(np.array(y, dtype=np.int32), device="cuda")
    got = _cluster_scores(Xd, labd, k)
    for key in ("cent", "mean", "intra"):
        assert not np.isnan(got[key]).any(), f"{key} has unwritten elements"
    np.testing.assert_array_equal(got["counts"], np.bincount(y, minlength=k))
    r = {key: _ratio(np.abs(got[key] - st[key]), st[key + "_bound"]) for key in ("cent", "mean", "intra", "db", "ch")}
    print("\n".join(f"RATIO {key} {name} {v:.4f}" for key, v in r.items()))
    for key, v in r.items():
        assert v <= 1.0, f"{key} outside its derived bound: {v} ({got[key] if key in ('db', 'ch') else ''} vs {st[key] if key in ('db', 'ch') else ''})"
    again = _cluster_scores(Xd, labd, k)
    for key in ("cent", "mean", "intra", "counts"):
        assert again[key].tobytes() == got[key].tobytes(), f"{key} differs on a second call"
    assert (again["db"], again["ch"]) == (got["db"], got["ch"])
    return got


@pytest.mark.parametrize("name", MC.CLU_IDS)
def test_cluster_score_kernels_within_derived_bounds(cuda, name):
    """Centroids, grand mean and mean intra-cluster distances (read back from the workspace), Davies-Bouldin and
    Calinski-Harabasz within the float64 rounding-count bounds of the longdouble oracle; counts equal to bincount;
    nothing left unwritten; a second call bit-identical."""
    X, y, k, st = _clu_reference(name)
    got = _check_cluster_scores(name, X, y, k, st)
    assert M.davies_bouldin_score(np.array(X), y) == got["db"] and M.calinski_harabasz_score(np.array(X), y) == got["ch"]


@pytest.mark.parametrize("name", list(MC.DEGENERATE))
def test_cluster_scores_sklearn_degenerate_branches(cuda, name):
    """sklearn's branches: a centroid distance of 0 contributes 0 (not inf), all intra distances 0 or all centroids
    coincident give Davies-Bouldin 0, zero intra-cluster dispersion gives Calinski-Harabasz 1 -- against the recorded
    sklearn values, live sklearn and the oracle (whose bounds are 0 where the value is a branch constant)."""
    from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score
    X, y, db, ch = MC.DEGENERATE[name]
    X, y = np.asarray(X, dtype=np.float32), np.asarray(y, dtype=np.int32)
    st = MT.cluster_stats(X, y)
    got = _check_cluster_scores(name, X, y, int(y.max()) + 1, st)
    assert got["db"] == pytest.approx(db, abs=1e-15) and got["ch"] == pytest.approx(ch, abs=1e-14)
    if db == 0.0:
        assert got["db"] == 0.0
    if ch in (0.0, 1.0):
        assert got["ch"] == ch
    assert got["db"] == pytest.approx(davies_bouldin_score(X, y), abs=1e-7)
    assert got["ch"] == pytest.approx(calinski_harabasz_score(X, y), abs=1e-7)
