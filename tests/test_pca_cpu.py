"""PCA checks that need no GPU: a float64 numpy restatement of both kernels stays inside the bounds of
tests/pca_check.py, the checker's exact PCA reproduces live sklearn and the recorded fixtures up to sklearn's own
float32 error with identical signs, the cases meet the gap condition their component comparisons rest on, the
hlmc_pca_* entry points validate their arguments without touching a device, and the Python surface rejects what it
does not implement."""
import ctypes as C
import inspect
import warnings

import numpy as np
import pytest
from sklearn.decomposition import PCA as SkPCA

from hlmc_amd import _lib as L
from tests import pca_check as K

SMALL = [c for c in K.CASE_NAMES if K.CASES[c]["n"] <= 300]


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_restated_cov_is_inside_the_bounds(name):
    ex = K.exact(name)
    if ex.n * ex.d * ex.d > 5e7:      # the row-by-row restatement of the two big shapes: their first 600 rows
        ex = K.Exact(ex.X[:600], 1)
    mean, G, parts = K.cov_restated(ex.X, np.random.default_rng(5))
    assert (np.abs(mean - ex.mean_ld) <= ex.delta).all()
    err = np.abs(G - ex.G_ld).astype(np.float64)
    print(name, "gram err/bound", float((err / ex.gram_bound).max()))
    assert (err <= ex.gram_bound).all()
    assert len(parts) == -(-ex.n // K.slab_len(ex.n))


@pytest.mark.parametrize("n", K.GRID_N)
def test_restated_cov_on_the_edge_grid(n):
    for d in (15, 65):
        X = K.grid_input(n, d)
        mean_ld, xc_ld, G_ld = K.exact_mean_gram(X)
        mean, G, _ = K.cov_restated(X)
        assert (np.abs(mean - mean_ld) <= K.mean_delta(X)).all()
        assert (np.abs(G - G_ld).astype(np.float64) <= K.gram_bound(X, xc_ld)).all()


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_restated_project_is_inside_the_bound(name):
    ex = K.exact(name)
    rows = ex.X[:100]
    got = K.project_restated(rows, ex.forward_matrix(), ex.mean, None)
    want, bound = K.project_exact(rows, ex.forward_matrix(), ex.mean, None)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    got = K.project_restated(want.astype(np.float32), ex.V, None, ex.mean)
    want2, bound2 = K.project_exact(want.astype(np.float32), ex.V, None, ex.mean)
    assert (np.abs(got.astype(np.float64) - want2) <= bound2).all()


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_gap_condition_and_rho(name):
    """Every compared component has a bound <= 1e-7; outside wide_all (rank n - 1, all 50 kept) that is all k."""
    ex = K.exact(name)
    fx = np.load(K.fixture_path(name))
    assert (ex.comp_bound[ex.comparable] <= K.COMPONENT_BOUND_MAX).all()
    if name != "wide_all":
        assert ex.comparable.all(), (name, ex.comp_bound.max())
    else:
        assert ex.comparable.sum() >= 40
    assert ex.k == int(fx["n_components"])
    assert abs(ex.rho - float(fx["rho"])) <= 0.5 * float(fx["rho"]) + 1e-13, (ex.rho, float(fx["rho"]))
    assert ex.E / ex.lam[0] < 1e-9


def _check_against_sklearn(ex, sk, T_sk, tag):
    """sklearn's float32 'full' solver against the exact PCA: the same signs, errors of float32 size."""
    f32 = 2.0 ** -23
    c = ex.comparable
    assert (np.sign(sk["components"][c]) == np.sign(ex.V[c]))[np.abs(ex.V[c]) > 1e-3].all(), tag
    assert np.abs(sk["components"][c] - ex.V[c]).max() <= 100 * f32, tag
    scale = ex.variance[0]
    assert np.abs(sk["explained_variance"] - ex.variance).max() <= 100 * f32 * scale, tag
    assert np.abs(sk["explained_variance_ratio"] - ex.ratio).max() <= 100 * f32, tag
    assert np.abs(sk["singular_values"] - ex.singular).max() <= 100 * f32 * ex.singular[0], tag
    assert abs(float(sk["noise_variance"]) - ex.noise) <= 100 * f32 * scale, tag
    assert np.abs(sk["mean"] - ex.mean).max() <= 8 * f32 * np.abs(ex.X).max(), tag      # a float32 sum of the column
    rows = T_sk.shape[0]
    want, _ = ex.transform(ex.X[:rows])
    tol = 100 * f32 * np.abs(want).max()
    assert np.abs(T_sk[:, c] - want[:, c]).max() <= tol, tag


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_exact_pca_reproduces_the_fixture(name):
    ex = K.exact(name)
    fx = np.load(K.fixture_path(name))
    assert ex.X.shape == (int(fx["n"]), int(fx["d"])) and str(fx["sklearn_version"]) == "1.7.2"
    _check_against_sklearn(ex, fx, fx["transform"], name)


@pytest.mark.parametrize("name", SMALL)
def test_exact_pca_reproduces_live_sklearn(name):
    ex = K.exact(name)
    c = K.CASES[name]
    sk = SkPCA(n_components=c["k"], svd_solver="full", whiten=c.get("whiten", False))
    T = sk.fit_transform(ex.X)
    attrs = dict(components=sk.components_, explained_variance=sk.explained_variance_,
                 explained_variance_ratio=sk.explained_variance_ratio_, singular_values=sk.singular_values_,
                 mean=sk.mean_, noise_variance=sk.noise_variance_)
    assert sk.n_components_ == ex.k
    _check_against_sklearn(ex, attrs, T[:K.FIXTURE_ROWS], name)


def test_constant_fixture_is_live_sklearn():
    X = K.case_input(K.CONSTANT)
    fx = np.load(K.fixture_path(K.CONSTANT))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = SkPCA(n_components=3, svd_solver="full").fit(X)
    assert np.array_equal(sk.components_, fx["components"]) and np.isnan(fx["explained_variance_ratio"]).all()
    assert not fx["explained_variance"].any() and not fx["singular_values"].any() and not fx["transform"].any()
    from hlmc_amd.decomposition import _eig_descending
    lam, V = _eig_descending(np.zeros((5, 5)))        # the host step on the Gram matrix such an input gives
    assert not lam.any() and np.array_equal(V[:3], fx["components"])


def test_host_eigen_step_matches_the_checker():
    from hlmc_amd.decomposition import _eig_descending
    ex = K.exact("full")
    lam, V = _eig_descending(ex.G)
    assert np.array_equal(lam, ex.lam_all) and np.array_equal(V, ex.V_all)
    assert (V[np.arange(16), np.argmax(np.abs(V), axis=1)] > 0).all()


def test_slab_geometry():
    assert K.slab_len(2) == 256 and K.slab_len(1336) == 256 and K.slab_len(128 * 256) == 256
    assert K.slab_len(128 * 256 + 1) == 288 and K.slab_len(100000) == 800 and K.slab_len(1 << 24) == 131072
    assert K.tile_pairs(129) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    lib = L.lib()
    for n, d in ((2, 1), (1336, 370), (100000, 128), (513, 129)):
        slabs = -(-n // K.slab_len(n))
        want = -(-slabs * d * 8 // 256) * 256 + slabs * len(K.tile_pairs(d)) * 64 * 64 * 8
        assert lib.hlmc_pca_workspace(n, d) == want, (n, d)


def test_entry_points_reject_bad_arguments():
    lib = L.lib()
    one = C.c_void_p(256)          # non-null placeholders: validation fails before anything is dereferenced
    big = 1 << 40
    for n, d in ((1, 4), (0, 4), (-3, 4), ((1 << 24) + 1, 4), (100, 0), (100, 1025), (100, -1)):
        assert lib.hlmc_pca_workspace(n, d) == 0, (n, d)
    ws = lib.hlmc_pca_workspace(1000, 16)
    assert ws > 0 and lib.hlmc_pca_workspace(1 << 24, 1024) > 0
    bad_cov = [(dict(X=None), b"NULL"), (dict(mean=None), b"NULL"), (dict(G=None), b"NULL"), (dict(ws=None), b"NULL"),
               (dict(n=1), b"2 <= n"), (dict(n=(1 << 24) + 1), b"2 <= n"), (dict(d=0), b"1 <= d <= 1024"),
               (dict(d=1025), b"1 <= d <= 1024"), (dict(ws_bytes=ws - 1), b"workspace"),
               (dict(ws_bytes=-1), b"workspace")]
    for change, msg in bad_cov:
        a = dict(X=one, n=1000, d=16, mean=one, G=one, ws=one, ws_bytes=big)
        a.update(change)
        st = lib.hlmc_pca_cov(None, a["X"], a["n"], a["d"], a["mean"], a["G"], a["ws"], a["ws_bytes"])
        assert st == -1, change
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())
    bad_proj = [(dict(A=None), b"NULL"), (dict(B=None), b"NULL"), (dict(out=None), b"NULL"), (dict(n=0), b"1 <= n"),
                (dict(p=0), b"1 <= p <= 1024"), (dict(p=1025), b"1 <= p <= 1024"), (dict(q=0), b"1 <= q <= 1024"),
                (dict(q=1025), b"1 <= q <= 1024")]
    for change, msg in bad_proj:
        a = dict(A=one, n=100, p=16, B=one, q=4, out=one)
        a.update(change)
        st = lib.hlmc_pca_project(None, a["A"], a["n"], a["p"], a["B"], a["q"], None, None, a["out"])
        assert st == -1, change
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())
    with pytest.raises(L.HLMCError):
        L.check(lib.hlmc_pca_cov(None, one, 1, 16, one, one, one, big), "hlmc_pca_cov")


def test_python_surface():
    import hlmc_amd
    assert hlmc_amd.PCA is hlmc_amd.decomposition.PCA
    assert hlmc_amd.pca_kmeans_baseline is hlmc_amd.decomposition.pca_kmeans_baseline
    for kw in (dict(n_components="mle"), dict(svd_solver="randomized"), dict(svd_solver="arpack")):
        with pytest.raises(ValueError):
            hlmc_amd.PCA(**kw)
    for solver in ("auto", "full", "covariance_eigh"):
        hlmc_amd.PCA(3, svd_solver=solver, random_state=0)
    X = np.random.default_rng(0).normal(size=(10, 4)).astype(np.float32)
    for k in (0, 5, -1, 1.5, 1.0, 0.0):       # rejected before anything moves to a device
        with pytest.raises(ValueError):
            hlmc_amd.PCA(k).fit(X)
    with pytest.raises(ValueError):
        hlmc_amd.PCA(1).fit(X[:1])
    with pytest.raises(ValueError):
        hlmc_amd.PCA(1).fit(np.zeros((4, 1025), np.float32))
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[3, 2] = bad
        with pytest.raises(ValueError, match="Input X contains NaN or infinity"):
            hlmc_amd.PCA(2).fit(Y)
    ours = inspect.signature(hlmc_amd.PCA.__init__).parameters
    theirs = inspect.signature(SkPCA.__init__).parameters
    for name in ("n_components", "whiten", "svd_solver", "random_state"):
        assert ours[name].default == theirs[name].default, name
        assert ours[name].kind == theirs[name].kind, name
    m = hlmc_amd.PCA()
    assert (m.n_components, m.whiten, m.svd_solver, m.random_state, m.device) == (None, False, "auto", None, None)
