"""DBSCAN on the GPU vs sklearn 1.7.2: labels and core sample indices must be bit-identical to the recorded fixtures
and to a live ``sklearn.cluster.DBSCAN`` (``algorithm='brute'`` where d <= 15), the borderline-pair count must equal
the numpy checker's (tests/dbscan_check.py) and be 0 on every real-valued case, the exact-arithmetic cases (integer
lattice, bridge point) must be equal although their ties count as borderline, and the eps sweep must agree with
single fits and with the reference's search loop."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from sklearn.cluster import DBSCAN as SkDBSCAN

import hlmc_amd
from hlmc_amd import _lib as L
from tests import dbscan_check as K

pytestmark = pytest.mark.gpu


def sk_fit(X, eps, min_samples=K.MIN_SAMPLES):
    algorithm = "brute" if X.shape[1] <= 15 else "auto"
    return SkDBSCAN(eps=eps, min_samples=min_samples, algorithm=algorithm).fit(X)


@functools.lru_cache(maxsize=None)
def checked(name, i):
    """The checker's (labels, core, borderline pairs) of fixture case `name`, radius i: computed once."""
    fx = np.load(K.fixture_path(name))
    return K.dbscan(K.case_input(name), float(fx["eps"][i]), int(fx["min_samples"]))


def assert_same(db, labels, core, what):
    assert db.labels_.dtype == np.int64
    assert np.array_equal(db.labels_, labels), what
    assert np.array_equal(db.core_sample_indices_, core), what


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_labels_match_fixture_and_live_sklearn(cuda, name):
    fx = np.load(K.fixture_path(name))
    X = K.case_input(name)
    ms = int(fx["min_samples"])
    for i, eps in enumerate(fx["eps"]):
        db = hlmc_amd.DBSCAN(eps=float(eps), min_samples=ms).fit(X)
        assert_same(db, fx[f"labels_{i}"], fx[f"core_{i}"], (name, eps, "fixture"))
        sk = sk_fit(X, float(eps), ms)
        assert_same(db, sk.labels_, sk.core_sample_indices_, (name, eps, "live sklearn"))
        _, _, border = checked(name, i)
        print(f"{name} eps={eps}: borderline pairs checker {border}, gpu {db.n_borderline_pairs_}")
        assert border == 0
        assert db.n_borderline_pairs_ == border
        assert np.array_equal(db.components_, X[db.core_sample_indices_]) and db.n_features_in_ == X.shape[1]


def _normal(n, d, seed):
    return np.random.default_rng(seed).normal(0.0, 1.0, (n, d)).astype(np.float32)


def _two_groups(n, d, seed, gap=20.0):
    X = _normal(n, d, seed)
    X[n // 2:, 0] += gap
    return X


SHAPE_CASES = {
    # name: (X, eps, min_samples)
    "n1": (_normal(1, 16, 1), 1.0, 5),
    "n1_min_samples1": (_normal(1, 16, 1), 1.0, 1),
    "n63": (_two_groups(63, 16, 2), 5.2, 5),
    "n64": (_two_groups(64, 16, 3), 5.2, 5),
    "n65": (_two_groups(65, 16, 4), 5.2, 5),
    "n129": (_two_groups(129, 16, 5), 5.0, 5),
    "d1": (_two_groups(300, 1, 6), 0.02, 5),
    "d3": (_two_groups(300, 3, 7), 0.45, 5),
    "d130": (_two_groups(200, 130, 8), 15.6, 5),
    "all_noise": (_normal(150, 16, 9), 0.5, 5),
    "one_cluster_no_noise": (_normal(150, 16, 10), 50.0, 5),
    "duplicate_rows": (np.repeat(_two_groups(40, 16, 11), 4, axis=0), 4.6, 5),
    "min_samples1": (_two_groups(200, 16, 12), 4.6, 1),
}


@pytest.mark.parametrize("name", list(SHAPE_CASES))
def test_shape_edge_cases_match_live_sklearn(cuda, name):
    X, eps, ms = SHAPE_CASES[name]
    db = hlmc_amd.DBSCAN(eps=eps, min_samples=ms).fit(X)
    sk = sk_fit(X, eps, ms)
    clusters, noise, border_pts = K.stats(sk.labels_, sk.core_sample_indices_)
    print(f"{name}: clusters {clusters}, noise {noise}, border points {border_pts}")
    assert_same(db, sk.labels_, sk.core_sample_indices_, name)
    labels, core, border = K.dbscan(X, eps, ms)
    assert_same(db, labels, core, (name, "checker"))
    assert border == 0 and db.n_borderline_pairs_ == 0
    if name == "all_noise":
        assert (db.labels_ == -1).all() and db.core_sample_indices_.size == 0 and db.components_.shape == (0, 16)
    if name == "one_cluster_no_noise":
        assert (db.labels_ == 0).all()


@pytest.mark.parametrize("eps", [1.0, 2.0, 2 ** 0.5])
def test_integer_lattice_is_exact(cuda, eps):
    """Integer coordinates and thresholds: exact in any summation order, so equality is required although the ties
    (eps = 1, 2) are counted as borderline; eps = sqrt(2) must exclude the pairs at squared distance exactly 2."""
    X = K.lattice()
    db = hlmc_amd.DBSCAN(eps=eps, min_samples=5).fit(X)
    sk = sk_fit(X, eps)
    assert_same(db, sk.labels_, sk.core_sample_indices_, eps)
    labels, core, border = K.dbscan(X, eps)
    assert_same(db, labels, core, (eps, "checker"))
    assert db.n_borderline_pairs_ == border
    assert (border > 0) == (eps in (1.0, 2.0))


def test_bridge_point_under_permutations(cuda):
    X = K.bridge()
    rng = np.random.default_rng(1)
    for trial in range(8):
        p = rng.permutation(X.shape[0]) if trial else np.arange(X.shape[0])
        db = hlmc_amd.DBSCAN(eps=1.0, min_samples=5).fit(X[p])
        sk = sk_fit(X[p], 1.0)
        assert_same(db, sk.labels_, sk.core_sample_indices_, p)
        assert db.labels_[int(np.flatnonzero(p == 12)[0])] == 0
        assert db.n_borderline_pairs_ == K.dbscan(X[p], 1.0)[2] > 0


def _reference_search(X, eps_range, min_samples=5):
    """The reference's loop (src/Convolutional_VAE.py:347-374) over sklearn DBSCAN and this package's silhouette."""
    best_eps, best_sil = 5.0, -1
    for eps in eps_range:
        labels = sk_fit(X, eps, min_samples).labels_
        unique = set(labels)
        unique.discard(-1)
        if len(unique) >= 2:
            sil = hlmc_amd.metrics.silhouette_score(X, labels)
            if sil > best_sil:
                best_sil, best_eps = sil, eps
    return 10.0 if best_sil == -1 else best_eps


@pytest.mark.parametrize("cap", [None, 1])   # one chunk for all radii / a cap so small that every radius is its own chunk
def test_eps_sweep_matches_single_fits_and_reference_search(cuda, cap):
    X = K.case_input("blobs_n1000_d32")
    eps_range = np.arange(4.0, 13.0, 1.0)
    best, records = hlmc_amd.dbscan_eps_sweep(X, eps_range, min_samples=5, workspace_cap=cap)
    assert len(records) == len(eps_range)
    scored = 0
    for eps, rec in zip(eps_range, records):
        db = hlmc_amd.DBSCAN(eps=eps, min_samples=5).fit(X)
        assert rec["eps"] == eps and np.array_equal(rec["labels"], db.labels_), eps
        assert rec["labels"].dtype == np.int64 and rec["n_borderline_pairs"] == db.n_borderline_pairs_
        assert rec["n_clusters"] == len(set(db.labels_) - {-1}) and rec["n_noise"] == int((db.labels_ == -1).sum())
        if rec["n_clusters"] >= 2:
            assert rec["silhouette"] == hlmc_amd.metrics.silhouette_score(X, db.labels_)
            scored += 1
        else:
            assert rec["silhouette"] is None
    assert scored >= 2
    assert best == _reference_search(X, eps_range)
    assert best == max((r for r in records if r["silhouette"] is not None), key=lambda r: r["silhouette"])["eps"]


def test_eps_sweep_default_when_no_radius_qualifies(cuda):
    X = K.case_input("blobs_n777_d16")
    eps_range = [0.05, 0.1, 500.0]          # all noise, all noise, one cluster: nothing to score
    best, records = hlmc_amd.dbscan_eps_sweep(X, eps_range)
    assert best == 10.0 == _reference_search(X, eps_range)
    assert [r["n_clusters"] for r in records] == [0, 0, 1] and all(r["silhouette"] is None for r in records)


def test_two_runs_give_identical_bits(cuda):
    X = K.case_input("blobs_n2000_d128")
    eps = float(np.load(K.fixture_path("blobs_n2000_d128"))["eps"][0])
    a = hlmc_amd.DBSCAN(eps=eps).fit(X)
    b = hlmc_amd.DBSCAN(eps=eps).fit(torch.from_numpy(X).to(cuda))     # a device tensor is accepted as well
    assert a.labels_.tobytes() == b.labels_.tobytes()
    assert a.core_sample_indices_.tobytes() == b.core_sample_indices_.tobytes()
    assert a.n_borderline_pairs_ == b.n_borderline_pairs_
    sweep = [hlmc_amd.dbscan_eps_sweep(X, [eps, 14.0, 19.5])[1] for _ in range(2)]
    for ra, rb in zip(*sweep):
        assert ra["labels"].tobytes() == rb["labels"].tobytes() and ra["silhouette"] == rb["silhouette"]


def _neighbors_op(X, radii_sq, dev):
    """hlmc_dbscan_neighbors on its own: (counts int32 [E][n], borderline pairs [E])."""
    lib = L.lib()
    n, d = X.shape
    E = len(radii_sq)
    Xd = torch.from_numpy(X).to(dev)
    ws_bytes = int(lib.hlmc_dbscan_workspace(n, E))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.full((E, n), -1, dtype=torch.int32, device=dev)
    border = torch.full((E,), -1, dtype=torch.int64, device=dev)
    r = (C.c_double * E)(*radii_sq)
    L.check(lib.hlmc_dbscan_neighbors(L.stream(), Xd.data_ptr(), n, d, r, E, counts.data_ptr(), border.data_ptr(),
                                      ws.data_ptr(), ws_bytes), "hlmc_dbscan_neighbors")
    return counts.cpu().numpy(), border.cpu().numpy()


# the tile edge on both grid axes x the K tail, chunk + 1 and several chunks + 2; one case with all 32 radii
NEIGHBOR_SHAPES = [(n, d, None) for n in (1, 63, 64, 65, 129) for d in (1, 3, 4, 5, 33, 130)] + [(65, 5, 32)]


@pytest.mark.parametrize("n,d,E", NEIGHBOR_SHAPES)
def test_neighbors_op_counts_and_ties_are_exact(cuda, n, d, E):
    """Integer-valued rows: every product and sum is exact in float64 in any order, so the op's neighbour counts and
    borderline-pair counts (here: the exact ties |x_i - x_j|^2 == r) equal the numpy checker's, no tolerance.  Radii:
    a tie value, a value no distance takes, a mid-range one."""
    X = np.random.default_rng(1000 * n + d).integers(0, 4, (n, d)).astype(np.float32)
    radii = [1.0, 2.5, 0.75 * d] if E is None else [0.5 * (e + 1) for e in range(E)]
    counts, border = _neighbors_op(X, radii, cuda)
    d2, norms = K.sq_distances(X)
    tol = (4.0 * (d + 4) * 2.0 ** -53) * (norms[:, None] + norms[None, :])    # dbscan_check.neighbourhoods
    for e, r in enumerate(radii):
        assert np.array_equal(counts[e], (d2 <= r).sum(axis=1)), (n, d, r)
        assert int(border[e]) == int(np.triu(np.abs(d2 - r) <= tol, k=1).sum()), (n, d, r)
        assert (int(counts[e].sum()) - n) % 2 == 0, (n, d, r)     # every pair is seen from both sides
