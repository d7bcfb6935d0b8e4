"""The hlmc_km_* entry points validate their arguments on the host, ahead of any launch: every case below passes
placeholder pointers, so it must come back with status -1 (HLMC_EINVAL) and the matching hlmc_last_error() without a
device being touched.  A case that reached a launch would be a hole in the validation (csrc/kmeans.hip)."""
import ctypes as C

import pytest

from hlmc_amd import _lib as L

ONE = C.c_void_p(256)          # non-null placeholder: validation fails before anything is dereferenced
BIG = 1 << 40


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _f64(*v):
    return (C.c_double * len(v))(*v)


def _reject(call, base, cases):
    lib = L.lib()
    for change, msg in cases:
        a = dict(base)
        a.update(change)
        st = call(lib, a)
        assert st == -1, (change, st, lib.hlmc_last_error())
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())


def _nulls(*names):
    return [({n: None}, b"arguments") for n in names]


def test_center_rejects_bad_arguments():
    _reject(lambda lib, a: lib.hlmc_km_center(None, a["X"], a["n"], a["d"], a["mean"], ONE, a["Xc"]),
            dict(X=ONE, n=100, d=8, mean=ONE, Xc=ONE),
            _nulls("X", "mean", "Xc") + [(dict(n=0), b"arguments"), (dict(d=0), b"arguments"),
                                         (dict(n=1 << 30), b"n too large")])


def test_sqdist_rows_rejects_bad_arguments():
    ok = L.i64_array([0, 99])
    _reject(lambda lib, a: lib.hlmc_km_sqdist_rows(None, a["X"], a["n"], a["d"], a["cand"], a["ncand"], a["out"]),
            dict(X=ONE, n=100, d=8, cand=ok, ncand=2, out=ONE),
            _nulls("X", "cand", "out") + [
                (dict(ncand=0), b"km_sqdist_rows arguments"), (dict(ncand=17, cand=L.i64_array([0] * 17)), b"arguments"),
                (dict(d=513), b"km_sqdist_rows arguments"), (dict(n=0), b"km_sqdist_rows sizes"),
                (dict(n=-5), b"km_sqdist_rows sizes"), (dict(d=0), b"km_sqdist_rows sizes"),
                (dict(d=-1), b"km_sqdist_rows sizes"),
                (dict(cand=L.i64_array([0, 100])), b"candidate index out of range"),
                (dict(cand=L.i64_array([-1, 5])), b"candidate index out of range")])


def test_assign_rejects_bad_arguments():
    sizes = [(dict(n=0), b"km_assign arguments"), (dict(d=0), b"km_assign arguments"),
             (dict(k=0), b"km_assign arguments"),
             (dict(k=400, d=128), b"too large for LDS")]      # (400 * 129 + 400 + 64 * 129) * 4 bytes > 160 KiB
    base = dict(X=ONE, n=1000, d=16, C=ONE, k=5, R=3, active=7, labels=ONE)
    _reject(lambda lib, a: lib.hlmc_km_assign_batch(None, a["X"], a["n"], a["d"], a["C"], a["k"], a["R"], a["active"],
                                                    a["labels"], ONE, ONE),
            base, _nulls("X", "C", "labels") + sizes + [(dict(R=0), b"km_assign arguments"),
                                                        (dict(R=65), b"km_assign arguments"),
                                                        (dict(R=-1), b"km_assign arguments")])
    _reject(lambda lib, a: lib.hlmc_km_assign(None, a["X"], a["n"], a["d"], a["C"], a["k"], a["labels"], None, None),
            base, _nulls("X", "C", "labels") + sizes)


def test_sums_reject_bad_arguments():
    lib = L.lib()
    n, k, R = 5000, 7, 3
    ws = int(lib.hlmc_km_sums_workspace(n, k))
    assert ws >= 4 * n and ws % 256 == 0
    base = dict(X=ONE, n=n, d=16, labels=ONE, k=k, R=R, active=7, sums=ONE, w=ONE, ws=ONE, ws_bytes=R * ws)
    common = _nulls("X", "labels", "sums", "w") + [(dict(k=0), b"arguments")]
    _reject(lambda lib, a: lib.hlmc_km_sums(None, a["X"], a["n"], a["d"], a["labels"], a["k"], a["sums"], a["w"]),
            base, common + [(dict(n=0), b"km_sums sizes"), (dict(d=0), b"km_sums sizes"),
                            (dict(n=1 << 30), b"km_sums sizes"), (dict(k=65536), b"km_sums sizes")])
    part = common + [({"ws": None}, b"arguments"), (dict(d=0), b"km_sums_part arguments"),
                     (dict(n=0), b"km_sums_part sizes"), (dict(n=1 << 30, ws_bytes=BIG), b"km_sums_part sizes"),
                     (dict(k=8193, ws_bytes=BIG), b"km_sums_part sizes")]
    _reject(lambda lib, a: lib.hlmc_km_sums_batch(None, a["X"], a["n"], a["d"], a["labels"], a["k"], a["R"], a["active"],
                                                  a["sums"], a["w"], a["ws"], a["ws_bytes"]),
            base, part + [(dict(R=0), b"km_sums_part arguments"), (dict(R=65, ws_bytes=BIG), b"km_sums_part arguments"),
                          (dict(ws_bytes=R * ws - 1), b"workspace too small"),      # one byte short
                          (dict(ws_bytes=ws), b"workspace too small"),              # one restart's worth for three
                          (dict(ws_bytes=-1), b"workspace too small")])
    _reject(lambda lib, a: lib.hlmc_km_sums_part(None, a["X"], a["n"], a["d"], a["labels"], a["k"], a["sums"], a["w"],
                                                 a["ws"], a["ws_bytes"]),
            dict(base, ws_bytes=ws), part + [(dict(ws_bytes=ws - 1), b"workspace too small")])


@pytest.mark.parametrize("k", [1, 2, 10, 8192])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4097, 100000])
def test_sums_workspace_closed_form(n, k):
    """One restart's partition workspace is the documented carve, int32 and packed -- hist and base [tiles][k] with
    tiles = ceil(n / 1024), off [k + 1], order [n] -- rounded up to 256 bytes once, at the end."""
    tiles = -(-n // 1024)
    packed = 4 * (2 * tiles * k + k + 1 + n)
    assert L.lib().hlmc_km_sums_workspace(n, k) == -(-packed // 256) * 256


def test_update_rejects_bad_arguments():
    _reject(lambda lib, a: lib.hlmc_km_update_batch(None, a["k"], a["d"], a["R"], 1, a["sums"], a["w"], a["C_old"],
                                                    a["C_new"], a["info"]),
            dict(k=5, d=16, R=3, sums=ONE, w=ONE, C_old=ONE, C_new=ONE, info=ONE),
            _nulls("sums", "w", "C_old", "C_new", "info") + [(dict(k=0), b"km_update arguments"),
                                                             (dict(d=0), b"km_update arguments"),
                                                             (dict(R=0), b"km_update arguments"),
                                                             (dict(R=65), b"km_update arguments")])


def test_pp_search_rejects_bad_arguments():
    best, rv = _i32(*([1] * 64)), _f64(*([0.5] * 64))
    _reject(lambda lib, a: lib.hlmc_km_pp_search(None, a["n"], a["R"], a["T"], a["prev"], a["prevT"], a["best"],
                                                 a["rv"], a["cand"], a["amb"]),
            dict(n=1000, R=3, T=4, prev=ONE, prevT=2, best=best, rv=rv, cand=ONE, amb=ONE),
            _nulls("prev", "best", "rv", "cand", "amb") + [
                (dict(n=0), b"km_pp_search arguments"), (dict(prevT=0), b"km_pp_search arguments"),
                (dict(R=0), b"outside [1, 64]"), (dict(T=0), b"outside [1, 64]"), (dict(R=65, T=1), b"outside [1, 64]"),
                (dict(R=5, T=13), b"outside [1, 64]"),                   # R * T = 65
                (dict(R=1, T=65), b"outside [1, 64]"),
                (dict(R=1 << 16, T=1 << 16), b"outside [1, 64]"),        # R * T wraps to 0 in int
                (dict(best=_i32(1, 2, 0)), b"best row out of range"),    # best[1] == prevT
                (dict(best=_i32(0, 0, -1)), b"best row out of range")])


def test_pp_dist_rejects_bad_arguments():
    best = _i32(*([1] * 64))
    _reject(lambda lib, a: lib.hlmc_km_pp_dist(None, a["X"], a["n"], a["d"], a["R"], a["T"], a["cand"], a["prev"],
                                               a["prevT"], a["best"], a["out"]),
            dict(X=ONE, n=1000, d=16, R=3, T=4, cand=ONE, prev=ONE, prevT=2, best=best, out=ONE),
            _nulls("X", "cand", "out") + [
                (dict(n=0), b"km_pp_dist arguments"), (dict(d=0), b"km_pp_dist arguments"),
                (dict(R=0), b"outside [1, 64]"), (dict(T=0), b"outside [1, 64]"), (dict(R=65, T=1), b"outside [1, 64]"),
                (dict(R=13, T=5), b"outside [1, 64]"), (dict(R=1 << 16, T=1 << 16), b"outside [1, 64]"),
                (dict(R=16, T=4, d=512), b"too large for LDS"),          # 64 * 513 doubles > 160 KiB
                (dict(best=None), b"prev needs best rows"), (dict(prevT=0), b"prev needs best rows"),
                (dict(best=_i32(1, 1, 2)), b"best row out of range"),
                (dict(best=_i32(-1, 1, 1)), b"best row out of range")])


def test_kmeans_rejects_non_finite_and_misshapen_input():
    """KMeans.fit / predict raise on NaN or infinity, as sklearn's check_array does, before any kernel runs (here:
    on CPU tensors, with no device at all).  A non-finite centre would leave the E-step without a cluster index to
    store, and the kernels after it index the centres with the labels unchecked."""
    import numpy as np
    import hlmc_amd
    X = np.random.default_rng(0).normal(0, 1, (50, 5)).astype(np.float32)
    km = hlmc_amd.KMeans(2, random_state=0, device="cpu")
    km.cluster_centers_ = X[:2].copy()
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[49, 4] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            km.fit(Xb)
        with pytest.raises(ValueError, match="NaN or infinity"):
            km.predict(Xb)
    with pytest.raises(ValueError, match="2-D"):
        km.fit(X[0])
    with pytest.raises(ValueError, match="features"):
        km.predict(X[:, :4])


def test_input_gate_checks_the_float32_values():
    """A float64 tensor holding a finite value above float32's range becomes infinity in the float32 matrix the
    kernels read, so every estimator that asks for finite input rejects it (on CPU tensors: no device is touched);
    the gate that does not ask (DBSCAN, the metrics) passes it through as infinity."""
    import numpy as np
    import torch
    import hlmc_amd
    X = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (50, 5)))     # float64
    ok = L.device_matrix(X, "cpu", finite=True)
    assert ok.dtype == torch.float32 and ok.is_contiguous() and torch.equal(ok, X.to(torch.float32))
    for big in (1e300, -1e300, 3.5e38):
        Xb = X.clone()
        Xb[7, 3] = big
        assert bool(torch.isfinite(Xb).all())
        with pytest.raises(ValueError, match="NaN or infinity"):
            L.device_matrix(Xb, "cpu", finite=True)
        km = hlmc_amd.KMeans(2, random_state=0, device="cpu")
        km.cluster_centers_ = X[:2].numpy().astype(np.float32)
        with pytest.raises(ValueError, match="NaN or infinity"):
            km.fit(Xb)
        with pytest.raises(ValueError, match="NaN or infinity"):
            km.predict(Xb)
        with pytest.raises(ValueError, match="NaN or infinity"):
            hlmc_amd.AgglomerativeClustering(n_clusters=2, device="cpu").fit(Xb)
        with pytest.raises(ValueError, match="NaN or infinity"):
            hlmc_amd.PCA(2, device="cpu").fit(Xb)
        assert not bool(torch.isfinite(L.device_matrix(Xb, "cpu")).all())


def test_inertia_and_rowdist_reject_bad_arguments():
    base = dict(X=ONE, n=1000, d=16, C=ONE, k=5, labels=ONE, R=3, out=ONE, tmp=ONE)
    sizes = [(dict(n=0), b"sizes"), (dict(n=-1), b"sizes"), (dict(d=0), b"sizes"), (dict(d=-4), b"sizes")]
    _reject(lambda lib, a: lib.hlmc_km_inertia_batch(None, a["X"], a["n"], a["d"], a["C"], a["k"], a["labels"], a["R"],
                                                     a["out"], a["tmp"]),
            base, _nulls("X", "C", "labels", "out", "tmp") + sizes + [
                (dict(k=0), b"km_inertia sizes"), (dict(R=0), b"km_inertia sizes"), (dict(R=65), b"km_inertia sizes"),
                (dict(R=-2), b"km_inertia sizes")])
    _reject(lambda lib, a: lib.hlmc_km_inertia(None, a["X"], a["n"], a["d"], a["C"], a["labels"], a["out"], a["tmp"]),
            base, _nulls("X", "C", "labels", "out", "tmp") + sizes)
    _reject(lambda lib, a: lib.hlmc_km_rowdist(None, a["X"], a["n"], a["d"], a["C"], a["labels"], a["out"]),
            base, _nulls("X", "C", "labels", "out") + sizes)
    with pytest.raises(L.HLMCError, match="km_rowdist"):
        L.check(L.lib().hlmc_km_rowdist(None, None, 10, 4, ONE, ONE, ONE), "hlmc_km_rowdist")
