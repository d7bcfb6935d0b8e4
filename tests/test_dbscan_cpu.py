"""DBSCAN checks that need no GPU: the numpy restatement of the rules (tests/dbscan_check.py) reproduces sklearn
1.7.2's recorded labels and core samples exactly, the float32-squared threshold and the bridge-point rule hold, and
the hlmc_dbscan_* entry points validate their arguments without touching a device."""
import ctypes as C

import numpy as np
import pytest

from hlmc_amd import _lib as L
from tests import dbscan_check as K


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_checker_reproduces_fixture(name):
    fx = np.load(K.fixture_path(name))
    X = K.case_input(name)
    assert X.shape == (int(fx["n"]), int(fx["d"]))
    rich = False
    for i, eps in enumerate(fx["eps"]):
        labels, core, border = K.dbscan(X, float(eps), int(fx["min_samples"]))
        assert np.array_equal(labels, fx[f"labels_{i}"]), (name, eps)
        assert np.array_equal(core, fx[f"core_{i}"]), (name, eps)
        assert border == 0, (name, eps, border)   # no summation order can flip a decision: equal by construction
        clusters, noise, n_border = K.stats(labels, core)
        rich |= clusters >= 2 and noise >= 1 and n_border >= 20
    assert rich, f"{name}: no radius with >= 2 clusters, >= 1 noise point and >= 20 border points"


def test_threshold_is_the_float32_square():
    """eps = sqrt(2): float32(eps)^2 in float32 is 1.9999999 < 2, so lattice pairs at squared distance exactly 2
    are NOT neighbours (they would be with eps^2 in float64 = 2.0000000000000004); eps = 1 and 2 keep exact ties."""
    assert K.radius_sq(2 ** 0.5) < 2.0 < (2 ** 0.5) ** 2
    assert K.radius_sq(1.0) == 1.0 and K.radius_sq(2.0) == 4.0
    X = K.lattice()
    d2, _ = K.sq_distances(X)
    at2, at1 = d2 == 2.0, d2 == 1.0
    assert at2.any() and at1.any()
    adj, _ = K.neighbourhoods(X, 2 ** 0.5)
    assert not adj[at2].any() and adj[at1].all()
    assert np.array_equal(adj, K.neighbourhoods(X, 1.0)[0])
    assert K.neighbourhoods(X, 1.0)[0][at1].all()
    assert K.neighbourhoods(X, 2.0)[0][d2 == 4.0].all()
    labels_a, core_a, _ = K.dbscan(X, 2 ** 0.5)
    labels_b, core_b, _ = K.dbscan(X, 1.0)
    assert np.array_equal(labels_a, labels_b) and np.array_equal(core_a, core_b)


def test_bridge_point_takes_the_smallest_cluster_number():
    X = K.bridge()
    rng = np.random.default_rng(0)
    for trial in range(40):
        p = rng.permutation(X.shape[0]) if trial else np.arange(X.shape[0])
        labels, core, _ = K.dbscan(X[p], 1.0)
        pos = {int(orig): int(new) for new, orig in enumerate(p)}
        ca, cb, br = pos[0], pos[6], pos[12]       # the two cross centres (the only cores) and the bridge
        assert sorted(core) == sorted([ca, cb])
        assert labels[min(ca, cb)] == 0 and labels[max(ca, cb)] == 1   # numbered by smallest core index
        assert labels[br] == 0                                           # adjacent to both: the smaller number
        assert (labels >= 0).all()


def test_entry_points_reject_bad_arguments():
    lib = L.lib()
    one = C.c_void_p(256)          # non-null placeholders: validation fails before anything is dereferenced
    r = (C.c_double * 2)(1.0, 4.0)
    big = 1 << 40
    assert lib.hlmc_dbscan_workspace(0, 1) == 0 and lib.hlmc_dbscan_workspace(10, 0) == 0
    assert lib.hlmc_dbscan_workspace(10, 33) == 0
    ws = lib.hlmc_dbscan_workspace(1000, 2)
    assert ws >= 2 * 1000 * 16 * 8
    bad_neighbors = [
        (dict(n=0), b"n"), (dict(d=0), b"d >= 1"), (dict(E=0), b"E"), (dict(E=33), b"E"),
        (dict(X=None), b"NULL"), (dict(r=None), b"NULL"), (dict(counts=None), b"NULL"), (dict(border=None), b"NULL"),
        (dict(ws=None), b"NULL"), (dict(ws_bytes=ws - 1), b"workspace"), (dict(ws_bytes=-1), b"workspace"),
    ]
    for change, msg in bad_neighbors:
        a = dict(X=one, n=1000, d=16, r=r, E=2, counts=one, border=one, ws=one, ws_bytes=big)
        a.update(change)
        st = lib.hlmc_dbscan_neighbors(None, a["X"], a["n"], a["d"], a["r"], a["E"], a["counts"], a["border"], a["ws"],
                                       a["ws_bytes"])
        assert st == -1, change
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())
    neg = (C.c_double * 2)(1.0, -1.0)
    assert lib.hlmc_dbscan_neighbors(None, one, 1000, 16, neg, 2, one, one, one, big) == -1
    bad_labels = [
        (dict(n=0), b"n"), (dict(E=0), b"E"), (dict(e=2), b"e < E"), (dict(e=-1), b"e < E"),
        (dict(min_samples=0), b"min_samples"), (dict(counts=None), b"NULL"), (dict(ws=None), b"NULL"),
        (dict(labels=None), b"NULL"), (dict(core=None), b"NULL"), (dict(ws_bytes=ws - 1), b"workspace"),
    ]
    for change, msg in bad_labels:
        a = dict(n=1000, E=2, e=0, min_samples=5, counts=one, ws=one, ws_bytes=big, labels=one, core=one)
        a.update(change)
        st = lib.hlmc_dbscan_labels(None, a["n"], a["E"], a["e"], a["min_samples"], a["counts"], a["ws"], a["ws_bytes"],
                                    a["labels"], a["core"], None)
        assert st == -1, change
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())
    with pytest.raises(L.HLMCError):
        L.check(lib.hlmc_dbscan_labels(None, 1000, 2, 0, 0, one, one, big, one, one, None), "hlmc_dbscan_labels")


def test_python_surface_rejects_other_metrics():
    import hlmc_amd
    with pytest.raises(ValueError):
        hlmc_amd.DBSCAN(eps=1.0, metric="manhattan")
    assert hlmc_amd.DBSCAN is hlmc_amd.cluster.DBSCAN and callable(hlmc_amd.dbscan_eps_sweep)
