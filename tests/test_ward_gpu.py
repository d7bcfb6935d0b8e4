"""Ward agglomerative clustering on the GPU vs sklearn 1.7.2.  Every comparison is exact: the distance matrix and the
raw merge records bit-equal to the numpy restatement (tests/ward_check.py), ``children_`` and ``labels_`` (k = 2..14)
equal and ``distances_`` bit-equal to the recorded fixtures and to a live ``sklearn.cluster.AgglomerativeClustering``,
and the k sweep equal to single fits and to the reference's selection rule."""
import functools
import warnings

import numpy as np
import pytest
import torch
from sklearn.cluster import AgglomerativeClustering as SkAgglomerative

import hlmc_amd
from hlmc_amd import _lib as L
from tests import ward_check as K

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. distances
def _pdist_input(n, d):
    return (np.random.default_rng(1000 * n + d).normal(0.0, 1.0, (n, d)) + 1000.0).astype(np.float32)


def _gpu_pdist(X, dev):
    n, d = X.shape
    Xd = torch.from_numpy(X).to(dev)
    D = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev)
    L.check(L.lib().hlmc_ward_pdist(L.stream(), Xd.data_ptr(), n, d, D.data_ptr()), "hlmc_ward_pdist")
    return D.cpu().numpy()


@pytest.mark.parametrize("d", [1, 3, 33, 128, 130])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 129, 257])
def test_pdist_is_bit_equal_to_the_restatement(cuda, n, d):
    X = _pdist_input(n, d)
    D = _gpu_pdist(X, cuda)
    want = K.pdist_full(X)
    bad = int((D.view(np.uint64) != want.view(np.uint64)).sum())
    print(f"pdist n={n} d={d}: {bad} of {n * n} elements differ in bits")
    assert bad == 0
    assert np.array_equal(D, D.T) and not D.diagonal().any()


# ------------------------------------------------------------------------------------------------ 2. the chain
def _gpu_chain(D, dev):
    """(status, ma, mb, md, ms, status word) of hlmc_ward_chain on a copy of D placed in the workspace."""
    lib = L.lib()
    n = D.shape[0]
    ws_bytes = int(lib.hlmc_ward_workspace(n))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    ws[:n * n * 8].copy_(torch.from_numpy(np.ascontiguousarray(D, dtype=np.float64)).view(torch.uint8).reshape(-1))
    ab = torch.full((3, n - 1), -7, dtype=torch.int32, device=dev)
    md = torch.full((n - 1,), float("nan"), dtype=torch.float64, device=dev)
    st = lib.hlmc_ward_chain(L.stream(), n, ws.data_ptr(), ab[0].data_ptr(), ab[1].data_ptr(), md.data_ptr(),
                             ab[2].data_ptr(), ws.data_ptr(), ws_bytes)
    off = (n * n * 8 + 255) // 256 * 256
    word = int(ws[off:off + 4].cpu().numpy().view(np.int32)[0])
    ab_h = ab.cpu().numpy()
    return st, ab_h[0], ab_h[1], md.cpu().numpy(), ab_h[2], word


@functools.lru_cache(maxsize=None)
def _chain_cases():
    return K.chain_matrices()


@pytest.mark.parametrize("name", ["integer_ties", "all_equal", "duplicate_zeros", "n2", "n2500"])
def test_chain_merges_are_bit_equal_to_the_restatement(cuda, name):
    D = _chain_cases()[name]
    st, ma, mb, md, ms, word = _gpu_chain(D, cuda)
    assert st == 0 and word == 0, (st, word, L.lib().hlmc_last_error())
    wa, wb, wd, wsz = K.nn_chain(D)
    assert np.array_equal(ma, wa) and np.array_equal(mb, wb), name
    bad = int((md.view(np.uint64) != wd.view(np.uint64)).sum())
    print(f"chain {name}: {bad} of {len(wd)} merge heights differ in bits")
    assert bad == 0
    assert np.array_equal(ms, wsz), name


def test_chain_reports_nan_through_the_status_word(cuda):
    st, ma, mb, md, ms, word = _gpu_chain(K.nan_matrix(), cuda)
    assert st == -4 and word == 1          # HLMC_EDEVICE, "a scan found no neighbour"
    assert b"status 1" in L.lib().hlmc_last_error()
    assert (ma == -7).all() and (mb == -7).all() and (ms == -7).all() and np.isnan(md).all()   # stopped at scan 0
    # the library is usable afterwards
    st, ma, mb, md, ms, word = _gpu_chain(_chain_cases()["n2"], cuda)
    assert st == 0 and word == 0 and (ma[0], mb[0], md[0], ms[0]) == (0, 1, 3.5, 2)


# ------------------------------------------------------------------------------------------------ 3. the class
@functools.lru_cache(maxsize=None)
def _fit(name):
    X = K.case_input(name)
    return hlmc_amd.AgglomerativeClustering(n_clusters=2, compute_distances=True).fit(X)


def _labels_for(name, k):
    m = _fit(name)
    return hlmc_amd.cluster._ward_cut(m.children_, m.n_leaves_, k)


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_tree_and_labels_match_fixture(cuda, name):
    fx = np.load(K.fixture_path(name))
    X = K.case_input(name)
    n, d = X.shape
    m = _fit(name)
    assert m.children_.dtype == np.int64 and m.labels_.dtype == np.int64 and m.distances_.dtype == np.float64
    assert np.array_equal(m.children_, fx["children"]), name
    bad = int((m.distances_.view(np.uint64) != fx["distances"].view(np.uint64)).sum())
    print(f"{name}: {bad} of {n - 1} distances differ in bits")
    assert bad == 0
    assert (m.n_clusters_, m.n_leaves_, m.n_connected_components_, m.n_features_in_) == (2, n, 1, d)
    for i, k in enumerate(K.K_RANGE):
        fit = hlmc_amd.AgglomerativeClustering(n_clusters=k).fit(X)
        assert fit.n_clusters_ == k and np.array_equal(fit.labels_, fx["labels"][i]), (name, k)
        assert np.array_equal(fit.labels_, _labels_for(name, k)), (name, k)      # one tree cut k ways: the same


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_tree_and_labels_match_live_sklearn(cuda, name):
    X = K.case_input(name)
    m = _fit(name)
    for k in K.K_RANGE:
        sk = SkAgglomerative(n_clusters=k, compute_distances=True).fit(X)
        assert np.array_equal(m.children_, sk.children_), (name, k)
        assert m.distances_.tobytes() == sk.distances_.tobytes(), (name, k)
        assert np.array_equal(_labels_for(name, k), sk.labels_), (name, k)


def test_one_cluster_and_n_clusters(cuda):
    X = K.case_input("gauss_n257_d7")
    n = X.shape[0]
    one = hlmc_amd.AgglomerativeClustering(n_clusters=1).fit(X)
    assert not one.labels_.any() and one.n_clusters_ == 1 and not hasattr(one, "distances_")
    every = hlmc_amd.AgglomerativeClustering(n_clusters=n).fit(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # sklearn: "partial build of the tree" does not apply without connectivity
        sk = SkAgglomerative(n_clusters=n).fit(X)
    assert np.array_equal(every.labels_, sk.labels_) and sorted(every.labels_.tolist()) == list(range(n))
    assert np.array_equal(one.labels_, SkAgglomerative(n_clusters=1).fit(X).labels_)


def test_bad_input_is_rejected(cuda):
    X = K.case_input("gauss_n64_d1")
    for k in (0, 65):
        with pytest.raises(ValueError):
            hlmc_amd.AgglomerativeClustering(n_clusters=k).fit(X)
    with pytest.raises(ValueError):
        hlmc_amd.AgglomerativeClustering().fit(X[:1])
    bad = X.copy()
    bad[3, 0] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
        hlmc_amd.AgglomerativeClustering().fit(bad)
    with pytest.raises(ValueError):
        hlmc_amd.AgglomerativeClustering().fit(torch.zeros(32769, 1, device=cuda))


def test_device_tensor_and_second_run_give_identical_bits(cuda):
    X = K.case_input("gauss_n300_d64")
    a = _fit("gauss_n300_d64")
    b = hlmc_amd.AgglomerativeClustering(n_clusters=2, compute_distances=True).fit(torch.from_numpy(X).to(cuda))
    c = hlmc_amd.AgglomerativeClustering(n_clusters=2, compute_distances=True).fit(X)
    for o in (b, c):
        assert a.children_.tobytes() == o.children_.tobytes() and a.distances_.tobytes() == o.distances_.tobytes()
        assert a.labels_.tobytes() == o.labels_.tobytes()


# ------------------------------------------------------------------------------------------------ 4. the sweep
def test_k_sweep_matches_single_fits_and_reference_rule(cuda):
    X = K.case_input("latents")
    best, records = hlmc_amd.agglomerative_k_sweep(X)
    assert [r["k"] for r in records] == list(K.K_RANGE)
    want_best, want_sil = 2, -1
    for i, (k, rec) in enumerate(zip(K.K_RANGE, records)):
        assert rec["labels"].dtype == np.int64
        assert np.array_equal(rec["labels"], hlmc_amd.AgglomerativeClustering(n_clusters=k).fit_predict(X)), k
        sk_labels = SkAgglomerative(n_clusters=k).fit_predict(X)
        assert np.array_equal(rec["labels"], sk_labels), k
        sil = hlmc_amd.metrics.silhouette_score(X, sk_labels)
        assert rec["silhouette"] == sil, k
        if sil > want_sil:
            want_best, want_sil = k, sil
    assert best == want_best
    again = hlmc_amd.agglomerative_k_sweep(X)
    assert again[0] == best
    for ra, rb in zip(records, again[1]):
        assert ra["labels"].tobytes() == rb["labels"].tobytes() and ra["silhouette"] == rb["silhouette"]
