"""Ward checks that need no GPU: the numpy restatement of the rules (tests/ward_check.py) reproduces live sklearn 1.7.2
and its recorded fixtures exactly (children and labels equal, distances bit-equal), the hlmc_ward_* entry points
validate their arguments without touching a device, and the Python surface rejects what it does not implement."""
import ctypes as C
import functools

import numpy as np
import pytest
from sklearn.cluster import AgglomerativeClustering as SkAgglomerative

from hlmc_amd import _lib as L
from tests import ward_check as K


@functools.lru_cache(maxsize=None)
def restated(name):
    return K.ward(K.case_input(name))


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_checker_reproduces_fixture(name):
    fx = np.load(K.fixture_path(name))
    X = K.case_input(name)
    n = X.shape[0]
    assert X.shape == (int(fx["n"]), int(fx["d"]))
    children, distances = restated(name)
    assert np.array_equal(children, fx["children"]), name
    assert distances.tobytes() == fx["distances"].tobytes(), name
    for i, k in enumerate(K.K_RANGE):
        assert np.array_equal(K.cut(children, n, k), fx["labels"][i]), (name, k)


@pytest.mark.parametrize("name", [c for c in K.CASE_NAMES if K.CASES[c][1] <= 300])
def test_checker_reproduces_live_sklearn(name):
    X = K.case_input(name)
    n = X.shape[0]
    children, distances = restated(name)
    for k in (2, 7, 14):
        sk = SkAgglomerative(n_clusters=k, compute_distances=True).fit(X)
        assert np.array_equal(children, sk.children_), (name, k)
        assert distances.tobytes() == sk.distances_.tobytes(), (name, k)
        assert np.array_equal(K.cut(children, n, k), sk.labels_), (name, k)


def test_pdist_is_scipys():
    from scipy.spatial.distance import pdist, squareform
    for name in ("gauss_n257_d7", "blobs_n200_d128", "grid_n150_d3"):
        X = K.case_input(name)
        D = K.pdist_full(X)
        assert D.tobytes() == squareform(pdist(X.astype(np.float64))).tobytes(), name
        assert np.array_equal(D, D.T) and not D.diagonal().any()


def test_crafted_matrices_cover_the_tie_rules():
    """The chain tests' matrices do what they are for: a scan that ties with the chain predecessor, and zeros."""
    mats = K.chain_matrices()
    ma, mb, md, ms = K.nn_chain(mats["all_equal"])
    assert ms[-1] == 33 and (ma < mb).all()
    ma, mb, md, ms = K.nn_chain(mats["integer_ties"])
    assert ms[-1] == 97 and len(np.unique(md)) < len(md)
    ma, mb, md, ms = K.nn_chain(mats["duplicate_zeros"])
    assert (md == 0.0).sum() == 40
    ma, mb, md, ms = K.nn_chain(mats["n2"])
    assert (ma[0], mb[0], md[0], ms[0]) == (0, 1, 3.5, 2)
    with pytest.raises(ValueError):
        K.nn_chain(K.nan_matrix())


def test_entry_points_reject_bad_arguments():
    lib = L.lib()
    one = C.c_void_p(256)          # non-null placeholders: validation fails before anything is dereferenced
    big = 1 << 40
    assert lib.hlmc_ward_workspace(1) == 0 and lib.hlmc_ward_workspace(0) == 0 and lib.hlmc_ward_workspace(-5) == 0
    assert lib.hlmc_ward_workspace(32769) == 0
    assert lib.hlmc_ward_workspace(32768) >= 32768 * 32768 * 8 + 32768 * 4
    ws = lib.hlmc_ward_workspace(1000)
    assert ws >= 1000 * 1000 * 8 + 1000 * 4
    bad_pdist = [(dict(X=None), b"NULL"), (dict(D=None), b"NULL"), (dict(n=1), b"n <= 32768"),
                 (dict(n=32769), b"n <= 32768"), (dict(d=0), b"d >= 1")]
    for change, msg in bad_pdist:
        a = dict(X=one, n=1000, d=16, D=one)
        a.update(change)
        assert lib.hlmc_ward_pdist(None, a["X"], a["n"], a["d"], a["D"]) == -1, change
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())
    bad_chain = [(dict(D=None), b"NULL"), (dict(ma=None), b"NULL"), (dict(mb=None), b"NULL"), (dict(md=None), b"NULL"),
                 (dict(ms=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(n=1), b"n <= 32768"),
                 (dict(n=32769), b"n <= 32768"), (dict(ws_bytes=ws - 1), b"workspace"),
                 (dict(ws_bytes=-1), b"workspace")]
    for change, msg in bad_chain:
        a = dict(n=1000, D=one, ma=one, mb=one, md=one, ms=one, ws=one, ws_bytes=big)
        a.update(change)
        st = lib.hlmc_ward_chain(None, a["n"], a["D"], a["ma"], a["mb"], a["md"], a["ms"], a["ws"], a["ws_bytes"])
        assert st == -1, change
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())
    with pytest.raises(L.HLMCError):
        L.check(lib.hlmc_ward_pdist(None, one, 1000, 0, one), "hlmc_ward_pdist")


def test_python_surface_rejects_what_is_not_implemented():
    import hlmc_amd
    for kw in (dict(linkage="average"), dict(linkage="complete"), dict(metric="manhattan"), dict(metric="cosine"),
               dict(connectivity=np.eye(3)), dict(distance_threshold=1.0)):
        with pytest.raises(ValueError):
            hlmc_amd.AgglomerativeClustering(n_clusters=3, **kw)
    assert hlmc_amd.AgglomerativeClustering is hlmc_amd.cluster.AgglomerativeClustering
    assert callable(hlmc_amd.agglomerative_k_sweep)
    m = hlmc_amd.AgglomerativeClustering()
    assert (m.n_clusters, m.metric, m.linkage, m.compute_distances) == (2, "euclidean", "ward", False)


def test_host_relabel_and_cut_match_the_checker():
    """The package's host part (stable sort, union-find, heap cut) on the checker's raw merges of a tied case."""
    from hlmc_amd import cluster
    X = K.case_input("grid_n150_d3")
    n = X.shape[0]
    ma, mb, md, _ = K.nn_chain(K.pdist_full(X))
    children, distances = cluster._ward_relabel(ma, mb, md, n)
    want_children, want_distances = restated("grid_n150_d3")
    assert np.array_equal(children, want_children) and distances.tobytes() == want_distances.tobytes()
    for k in (1, 2, 9, 14, n):
        assert np.array_equal(cluster._ward_cut(children, n, k), K.cut(want_children, n, k)), k
    assert sorted(cluster._ward_cut(children, n, n).tolist()) == list(range(n))
