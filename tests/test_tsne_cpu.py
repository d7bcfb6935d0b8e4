"""t-SNE checks that need no GPU: the helper tests/tsne_check.py is pinned to live sklearn (neighbour sets, the
perplexity search bit for bit, the joint P, the gradient and KL of _barnes_hut_tsne at theta = 0, the update of
_gradient_descent), the numpy restatements of the kernels stay inside the helper's bounds, the hlmc_tsne_* entry points
validate their arguments without touching a device, and the Python surface rejects what it does not implement."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.manifold import TSNE as SkTSNE
from sklearn.manifold import _barnes_hut_tsne, _t_sne, _utils
from sklearn.neighbors import NearestNeighbors

from hlmc_amd import _lib as L
from tests import tsne_check as K

PINNED_KNN = ["n63_d3_k16", "n129_d3_k91", "n300_d128_k91", "offset_n129_d33_k16"]
SEARCH_CASES, search_input, grad_case = K.SEARCH_CASES, K.search_input, K.grad_case


@pytest.mark.parametrize("name", PINNED_KNN)
def test_exact_neighbour_sets_are_sklearn_brute_force(name):
    n, d, k, _ = K.KNN_CASES[name]
    X = K.knn_input(name)
    D = K.sqdist_exact(X)
    idx, _ = K.knn_from(D.astype(np.float64), k)
    assert not K.knn_ambiguous_rows(D, K.sqdist_bound(X), k).any()       # the seeds leave no row undecided
    sk = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(X).kneighbors(return_distance=False)
    for i in range(n):
        assert set(idx[i]) == set(sk[i]), (name, i)


@pytest.mark.parametrize("name", list(K.KNN_CASES))
def test_restated_knn_is_inside_the_bound(name):
    n, d, k, kind = K.KNN_CASES[name]
    X = K.knn_input(name)
    D, bound = K.sqdist_exact(X), K.sqdist_bound(X)
    want_idx, want_d = K.knn_from(D.astype(np.float64), k)
    idx, d2 = K.knn_restated(X, k)
    rows = np.arange(n)[:, None]
    assert (np.abs(d2 - D[rows, idx].astype(np.float64)) <= bound[rows, idx]).all()
    assert (np.diff(d2, axis=1) >= 0).all()
    if kind == "dups":
        assert (np.abs(d2 - want_d) <= np.take_along_axis(bound, want_idx.astype(np.int64), 1).max()).all()
    else:
        amb = K.knn_ambiguous_rows(D, bound, k)
        assert not amb.any()
        assert all(set(idx[i]) == set(want_idx[i]) for i in range(n))


@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_search_reference_is_sklearn_bit_for_bit(name):
    _, _, d32, perp = search_input(name)
    want = _utils._binary_search_perplexity(np.ascontiguousarray(d32), perp, 0)
    P, beta = K.search_reference(d32, perp)
    assert np.array_equal(np.asarray(want, np.float64), P)
    if name == "wide":
        assert (beta < 1e-3).all()
    if name == "narrow":
        assert (beta > 1e3).all()


@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_restated_search_takes_the_reference_branches(name):
    _, _, d32, perp = search_input(name)
    P_ref, beta_ref = K.search_reference(d32, perp)
    P, beta, border, steps = K.search_restated(d32, perp)
    assert not border.any()                       # the seeds leave no step undecided
    assert np.array_equal(beta, beta_ref)
    assert (np.abs(P - P_ref) <= K.cond_p_bound(P_ref, d32, beta_ref, d32.shape[1])).all()
    H = K.perplexity_of(d32, beta)
    ok = np.abs(H - np.log(perp)) <= K.SEARCH_TOL * (1 + 1e-9)
    if name == "p5":          # neighbours all at one distance: H = log k for every beta, the search runs out
        assert (steps[:40] == 100).all() and ok[steps < 100].all() and (steps < 100).sum() >= 20
        assert np.array_equal(P[0], np.full(d32.shape[1], 1.0 / d32.shape[1]))
    else:
        assert ok.all()


@pytest.mark.parametrize("name", ["p5", "p30", "wide"])
def test_joint_reference_is_sklearn(name):
    X, idx, d32, perp = search_input(name)
    n, k = idx.shape
    # sklearn searches on the rows in column order: feed the reference the same order, then the bits agree
    order = np.argsort(idx, axis=1, kind="stable")
    idx_s, d_s = np.take_along_axis(idx, order, 1), np.take_along_axis(d32, order, 1)
    D = sp.csr_matrix((d_s.astype(np.float64).ravel(), idx_s.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    want = sp.csr_matrix(_t_sne._joint_probabilities_nn(D, perp, 0))
    want.sort_indices()
    cond, _ = K.search_reference(d_s, perp)
    indptr, indices, values = K.joint_reference(idx_s, cond)
    assert np.array_equal(indptr, want.indptr) and np.array_equal(indices, want.indices)
    assert np.array_equal(values, want.data)
    # the distance order the device searches in changes the low bits only
    cond2, _ = K.search_reference(d32, perp)
    ip2, ix2, v2 = K.joint_reference(idx, cond2)
    assert np.array_equal(ip2, indptr) and np.array_equal(ix2, indices)
    assert (np.abs(v2 - values) <= 64 * (k + 16) * K.U * values).all()


@pytest.mark.parametrize("name", ["p5", "p30"])
def test_restated_joint_is_inside_the_bound(name):
    X, idx, d32, perp = search_input(name)
    n, k = idx.shape
    cond, _, _, _ = K.search_restated(d32, perp)
    cond_ref, _ = K.search_reference(d32, perp)
    indptr, indices, values = K.joint_restated(idx, cond)
    ip, ix, want = K.joint_reference(idx, cond_ref)
    assert np.array_equal(indptr, ip) and np.array_equal(indices, ix)
    assert (np.abs(values.astype(np.float64) - want) <= K.joint_value_bound(want, n, k)).all()
    assert abs(float(values.astype(np.float64).sum()) - 1.0) <= n * k * 2 * K.V
    M = sp.csr_matrix((values, indices, indptr), shape=(n, n)).toarray()
    assert np.array_equal(M, M.T)


@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("exag", [1.0, 12.0])
def test_gradient_reference_is_sklearn_at_theta_0(scale, exag):
    n = 257
    Y, indptr, indices, values = grad_case(n, scale)
    ref = K.GradRef(Y, indptr, indices, values, exag)
    forces = np.zeros((n, 2), np.float32)
    err = _barnes_hut_tsne.gradient((values * np.float32(exag)).astype(np.float32), Y, indices.astype(np.int64),
                                    indptr.astype(np.int64), forces, 0.0, 2, 0, dof=1, compute_error=True,
                                    num_threads=1)
    # sklearn adds the n terms of each sum in float32: (n + 32) v of the terms' magnitudes
    bound = 4.0 * (n + 32) * K.V * (ref.attr_abs + ref.rep_abs / ref.z)
    got = 4.0 * forces.astype(np.float64)
    print("sklearn gradient err/bound", float((np.abs(got - ref.grad) / bound).max()))
    assert (np.abs(got - ref.grad) <= bound).all()
    assert abs(err - ref.kl) <= (len(values) + 32) * K.V * ref.kl_abs     # its error sum is a C float as well


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_restated_gradient_is_inside_the_bounds(n):
    for scale, exag in ((1e-4, 12.0), (1.0, 1.0), (50.0, 1.0)):
        Y, indptr, indices, values = grad_case(n, scale)
        ref = K.GradRef(Y, indptr, indices, values, exag)
        grad, Z, kl, gnorm = K.gradient_restated(Y, indptr, indices, values, exag)
        assert (np.abs(grad.astype(np.float64) - ref.grad) <= ref.grad_bound).all()
        assert abs(Z - ref.Z) <= ref.Z_bound and abs(kl - ref.kl) <= ref.kl_bound
        assert abs(gnorm - ref.gnorm) <= ref.gnorm_bound
    assert K.repulsion_restated(Y).shape == (-(-n // 256), 3, n)


def test_update_transcription_is_sklearn_gradient_descent():
    rng = np.random.default_rng(3)
    p0 = rng.normal(0.0, 1e-4, 600).astype(np.float32)

    coef = np.linspace(0.0, 0.06, 600).astype(np.float32)

    def objective(p, *args, **kwargs):     # quadratic bowls of growing steepness: the steep ones overshoot (gains fall)
        return 0.0, (p * coef).astype(np.float32)

    for momentum, lr in ((0.5, 50.0), (0.8, 200.0)):
        want, _, it = _t_sne._gradient_descent(objective, p0.copy(), it=0, max_iter=4, n_iter_check=1,
                                               n_iter_without_progress=300, momentum=momentum, learning_rate=lr,
                                               min_gain=0.01, min_grad_norm=0.0, verbose=0, args=[], kwargs={})
        p, update, gains = p0.copy(), np.zeros_like(p0), np.ones_like(p0)
        for _ in range(4):
            p, update, gains = K.gradient_descent_step(p, update, gains, objective(p)[1], momentum, lr)
        assert it == 3 and np.array_equal(p, want)
        assert len(np.unique(gains)) > 2 and gains.min() < 0.5 and gains.max() > 1.3


def test_geometry_and_workspace():
    assert K.col_slab_len(2) == 256 and K.col_slab_len(1336) == 256 and K.col_slab_len(64 * 256) == 256
    assert K.col_slab_len(64 * 256 + 1) == 512 and K.col_slab_len(100000) == 1792 and K.col_slab_len(131072) == 2048
    lib = L.lib()
    for n, d, k in ((2, 1, 1), (1336, 64, 91), (100000, 128, 91), (131072, 4096, 512)):
        off = K.grad_workspace_offsets(n)
        total = lib.hlmc_tsne_workspace(n, d, k)
        assert total > off["end"], (n, d, k)
        assert lib.hlmc_tsne_workspace(n, 1, 1) < total or (d, k) == (1, 1)


def test_entry_points_reject_bad_arguments():
    lib = L.lib()
    one = C.c_void_p(256)          # non-null placeholders: validation fails before anything is dereferenced
    big = 1 << 50
    for n, d, k in ((1, 4, 1), (0, 4, 1), (-3, 4, 1), (131073, 4, 1), (100, 0, 5), (100, 4097, 5), (100, 4, 0),
                    (100, 4, 100), (1000, 4, 513), (100, 4, -1)):
        assert lib.hlmc_tsne_workspace(n, d, k) == 0, (n, d, k)
    ws = lib.hlmc_tsne_workspace(1000, 16, 91)
    assert ws > 0 and lib.hlmc_tsne_workspace(131072, 4096, 512) > 0

    def expect(fn, base, cases):
        for change, msg in cases:
            a = dict(base)
            a.update(change)
            st = fn(**a)
            assert st == -1, change
            assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())

    def knn(X, n, d, k, idx, d2, ws, ws_bytes):
        return lib.hlmc_tsne_knn(None, X, n, d, k, idx, d2, ws, ws_bytes)
    expect(knn, dict(X=one, n=1000, d=16, k=91, idx=one, d2=one, ws=one, ws_bytes=big),
           [(dict(X=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(d2=None), b"NULL"), (dict(ws=None), b"NULL"),
            (dict(n=1), b"2 <= n"), (dict(n=131073), b"2 <= n"), (dict(d=0), b"1 <= d"), (dict(d=4097), b"1 <= d"),
            (dict(k=0), b"1 <= k"), (dict(k=513), b"1 <= k"), (dict(k=1000), b"1 <= k"),
            (dict(ws_bytes=ws - 1), b"workspace"), (dict(ws_bytes=-1), b"workspace")])

    def aff(idx, d2, n, k, perp, beta, cond, indptr, indices, values, ws, ws_bytes):
        return lib.hlmc_tsne_affinities(None, idx, d2, n, k, perp, beta, cond, indptr, indices, values, ws, ws_bytes)
    ws_aff = lib.hlmc_tsne_workspace(1000, 1, 91)
    expect(aff, dict(idx=one, d2=one, n=1000, k=91, perp=30.0, beta=one, cond=one, indptr=one, indices=one, values=one,
                     ws=one, ws_bytes=big),
           [(dict(idx=None), b"NULL"), (dict(d2=None), b"NULL"), (dict(beta=None), b"NULL"), (dict(cond=None), b"NULL"),
            (dict(indptr=None), b"NULL"), (dict(indices=None), b"NULL"), (dict(values=None), b"NULL"),
            (dict(ws=None), b"NULL"), (dict(n=1), b"2 <= n"), (dict(n=131073), b"2 <= n"), (dict(k=0), b"1 <= k"),
            (dict(k=513), b"1 <= k"), (dict(k=1000), b"1 <= k"), (dict(perp=0.0), b"perplexity"),
            (dict(perp=float("nan")), b"perplexity"), (dict(perp=float("inf")), b"perplexity"),
            (dict(ws_bytes=ws_aff - 1), b"workspace"), (dict(ws_bytes=-1), b"workspace")])

    def grad(Y, n, indptr, indices, values, exag, g, stats, ws, ws_bytes):
        return lib.hlmc_tsne_gradient(None, Y, n, indptr, indices, values, exag, g, stats, 1, ws, ws_bytes)
    ws_grad = K.grad_workspace_offsets(1000)["end"]
    base = dict(Y=one, n=1000, indptr=one, indices=one, values=one, exag=1.0, g=one, stats=one, ws=one, ws_bytes=big)
    bad = [(dict(Y=None), b"NULL"), (dict(indptr=None), b"NULL"), (dict(indices=None), b"NULL"),
           (dict(values=None), b"NULL"), (dict(stats=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(n=1), b"2 <= n"),
           (dict(n=131073), b"2 <= n"), (dict(exag=0.0), b"exaggeration"), (dict(exag=float("nan")), b"exaggeration"),
           (dict(ws_bytes=ws_grad - 1), b"workspace"), (dict(ws_bytes=-1), b"workspace")]
    expect(grad, base, bad + [(dict(g=None), b"NULL")])

    def run(Y, n, indptr, indices, values, exag, stats, ws, ws_bytes, update=one, gains=one, momentum=0.5, lr=50.0,
            n_iter=1):
        return lib.hlmc_tsne_run(None, Y, update, gains, n, indptr, indices, values, exag, momentum, lr, n_iter, stats,
                                 ws, ws_bytes)
    del base["g"]
    expect(run, base, bad + [(dict(update=None), b"NULL"), (dict(gains=None), b"NULL"), (dict(momentum=1.0), b"momentum"),
                             (dict(momentum=-0.1), b"momentum"), (dict(lr=0.0), b"learning_rate"),
                             (dict(n_iter=0), b"n_iter"), (dict(n_iter=100001), b"n_iter")])
    with pytest.raises(L.HLMCError):
        L.check(lib.hlmc_tsne_knn(None, one, 1, 16, 1, one, one, one, big), "hlmc_tsne_knn")


def test_python_surface():
    import hlmc_amd
    assert hlmc_amd.TSNE is hlmc_amd.manifold.TSNE
    for kw in (dict(n_components=3), dict(n_components=1), dict(metric="cosine"), dict(metric="precomputed"),
               dict(method="exact"), dict(init="spectral"), dict(learning_rate=0.0), dict(max_iter=100)):
        with pytest.raises(ValueError):
            hlmc_amd.TSNE(**kw)
    hlmc_amd.TSNE(2, angle=0.2, random_state=0, init="random", learning_rate=200.0)
    X = np.random.default_rng(0).normal(size=(40, 4)).astype(np.float32)
    for perp in (40.0, 41.0, 1000):               # rejected before anything moves to a device
        with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
            hlmc_amd.TSNE(perplexity=perp).fit(X)
    with pytest.raises(ValueError):
        hlmc_amd.TSNE(perplexity=5).fit(X[0])
    with pytest.raises(ValueError):
        hlmc_amd.TSNE(perplexity=5).fit(np.zeros((40, 4097), np.float32))
    with pytest.raises(ValueError, match="neighbours"):
        hlmc_amd.TSNE(perplexity=171).fit(np.zeros((1000, 3), np.float32))
    with pytest.raises(ValueError, match="init has shape"):
        hlmc_amd.TSNE(perplexity=5, init=np.zeros((39, 2), np.float32)).fit(X)
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[3, 2] = bad
        with pytest.raises(ValueError, match="Input X contains NaN or infinity"):
            hlmc_amd.TSNE(perplexity=5).fit(Y)
    ours = inspect.signature(hlmc_amd.TSNE.__init__).parameters
    theirs = inspect.signature(SkTSNE.__init__).parameters
    for name in ("n_components", "perplexity", "early_exaggeration", "learning_rate", "max_iter",
                 "n_iter_without_progress", "min_grad_norm", "metric", "init", "random_state", "method", "angle"):
        assert ours[name].default == theirs[name].default, name
        assert ours[name].kind == theirs[name].kind, name
    assert hlmc_amd.manifold.n_neighbors_for(65, 30.0) == 64 and hlmc_amd.manifold.n_neighbors_for(1336, 30.0) == 91
