"""GPU PCA against the exact oracle and the derived bounds of tests/pca_check.py: hlmc_pca_cov and hlmc_pca_project op
by op (every case, the edge grid, determinism, symmetry, the documented slab partials), hlmc_amd.PCA end to end
(eigenpairs, fit_transform, transform, inverse_transform), a triangle check against sklearn's recorded 'full' output,
and the PCA + K-Means baseline.  Every test prints its worst |err| / bound as
``PCA_RATIO <quantity> <case> <ratio>``."""
import functools
import itertools

import numpy as np
import pytest
import torch

from hlmc_amd import _lib as L
from tests import pca_check as K

pytestmark = pytest.mark.gpu


def report(quantity, case, err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(np.max(ratio)) if ratio.size else 0.0
    print(f"PCA_RATIO {quantity} {case} {worst:.4f}")
    assert (err <= bound).all(), (quantity, case, worst)


def run_cov(X, dev):
    """(mean, G, colsum [S][d], part [S][P][64][64]) of one hlmc_pca_cov call, all on the host."""
    lib = L.lib()
    n, d = X.shape
    Xd = torch.as_tensor(X, device=dev).contiguous()
    ws_bytes = int(lib.hlmc_pca_workspace(n, d))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    mean = torch.empty(d, dtype=torch.float64, device=dev)
    G = torch.empty(d, d, dtype=torch.float64, device=dev)
    L.check(lib.hlmc_pca_cov(L.stream(), Xd.data_ptr(), n, d, mean.data_ptr(), G.data_ptr(), ws.data_ptr(), ws_bytes),
            "hlmc_pca_cov")
    slabs = -(-n // K.slab_len(n))
    pairs = K.tile_pairs(d)
    raw = ws.cpu().numpy()
    off = -(-slabs * d * 8 // 256) * 256
    colsum = raw[:slabs * d * 8].view(np.float64).reshape(slabs, d)
    part = raw[off:off + slabs * len(pairs) * 64 * 64 * 8].view(np.float64).reshape(slabs, len(pairs), 64, 64)
    return mean.cpu().numpy(), G.cpu().numpy(), colsum, part


def check_cov(X, dev, tag, oracle=None):
    n, d = X.shape
    mean_ld, xc_ld, G_ld = oracle if oracle is not None else K.exact_mean_gram(X)
    mean, G, colsum, part = run_cov(X, dev)
    report("mean", tag, np.abs(mean - mean_ld).astype(np.float64), K.mean_delta(X))
    report("gram", tag, np.abs(G - G_ld).astype(np.float64), K.gram_bound(X, xc_ld))
    assert G.tobytes() == G.T.copy().tobytes(), tag                 # symmetric bit for bit
    mean2, G2, _, _ = run_cov(X, dev)
    assert mean.tobytes() == mean2.tobytes() and G.tobytes() == G2.tobytes(), tag   # run to run
    # the documented workspace: slab column sums, and the slab partials summed in slab order give G
    s = np.zeros(d)
    for b in range(colsum.shape[0]):
        s = s + colsum[b]
    assert (s / n).tobytes() == mean.tobytes(), tag
    for p, (ti, tj) in enumerate(K.tile_pairs(d)):
        acc = np.zeros((64, 64))
        for b in range(part.shape[0]):
            acc = acc + part[b, p]
        hi, hj = min(64, d - 64 * ti), min(64, d - 64 * tj)
        want = G[64 * ti:64 * ti + hi, 64 * tj:64 * tj + hj]
        got = acc[:hi, :hj]
        keep = np.triu(np.ones((hi, hj), bool)) if ti == tj else np.ones((hi, hj), bool)
        assert np.array_equal(got[keep], want[keep]), (tag, ti, tj)
        assert not part[:, p, hi:, :].any() and not part[:, p, :, hj:].any(), (tag, ti, tj)   # the zero fill
    return mean, G


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_cov_cases(cuda, name):
    ex = K.exact(name)
    mean, G = check_cov(ex.X, cuda, name, (ex.mean_ld, ex.xc_ld, ex.G_ld))
    if name == "zero_col":
        assert mean[5] == 3.0 and not G[5].any() and not G[:, 5].any()


@pytest.mark.parametrize("n", K.GRID_N)
def test_cov_edge_grid(cuda, n):
    for d in K.GRID_D:
        check_cov(K.grid_input(n, d), cuda, f"n{n}_d{d}")


@pytest.mark.parametrize("p", (1, 3, 37, 370))
def test_project_op(cuda, p):
    lib = L.lib()
    rng = np.random.default_rng(100 + p)
    for q, n in itertools.product((1, 15, 16, 17, 64, 65), (1, 63, 64, 65)):
        A = (rng.normal(0.0, 1.0, (n, p)) + 3.0).astype(np.float32)
        B = rng.normal(0.0, 1.0, (p, q)) + 0.25          # asymmetric, no zero entries
        a_off = rng.normal(3.0, 1.0, p)
        o_off = rng.normal(0.0, 50.0, q)
        Ad, Bd = torch.as_tensor(A, device=cuda), torch.as_tensor(B, device=cuda)
        ad, od = torch.as_tensor(a_off, device=cuda), torch.as_tensor(o_off, device=cuda)
        worst, misrounded = 0.0, 0
        for use_a, use_o in itertools.product((False, True), (False, True)):
            out = torch.full((n, q), float("nan"), dtype=torch.float32, device=cuda)
            L.check(lib.hlmc_pca_project(L.stream(), Ad.data_ptr(), n, p, Bd.data_ptr(), q,
                                         ad.data_ptr() if use_a else None, od.data_ptr() if use_o else None,
                                         out.data_ptr()), "hlmc_pca_project")
            want, bound = K.project_exact(A, B, a_off if use_a else None, o_off if use_o else None)
            err = np.abs(out.cpu().numpy().astype(np.float64) - want)
            assert (err <= bound).all(), (p, q, n, use_a, use_o, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            misrounded += int((out.cpu().numpy() != want.astype(np.float32)).sum())
        print(f"PCA_RATIO project p{p}_q{q}_n{n} {worst:.4f}")
        print(f"PCA_MISROUNDED project p{p}_q{q}_n{n} {misrounded} of {4 * n * q}")


@functools.lru_cache(maxsize=None)
def fitted(name):
    import hlmc_amd
    c = K.CASES[name]
    model = hlmc_amd.PCA(c["k"], whiten=c.get("whiten", False))
    T = model.fit_transform(K.case_input(name))
    return model, T


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_fit_eigenpairs(cuda, name):
    ex = K.exact(name)
    model, _ = fitted(name)
    assert (model.n_components_, model.n_samples_, model.n_features_in_) == (ex.k, ex.n, ex.d)
    lam_dev = model._variance64 * (ex.n - 1)
    report("eigenvalue", name, np.abs(lam_dev - ex.lam), np.full(ex.k, ex.E))
    c = ex.comparable
    err = np.sqrt(((model._components64 - ex.V) ** 2).sum(axis=1))
    report("component", name, err[c], ex.comp_bound[c])
    report("mean32", name, np.abs(model.mean_.astype(np.float64) - ex.mean), ex.delta + K.half_spacing32(ex.mean))
    for attr in ("components_", "explained_variance_", "explained_variance_ratio_", "singular_values_", "mean_"):
        assert getattr(model, attr).dtype == np.float32, attr
    assert np.array_equal(model.components_, model._components64.astype(np.float32))
    if name in ("full", "wide_all"):       # orthonormal rows: |v'_i . v'_j - delta_ij| <= cb_i + cb_j + cb_i cb_j
        V = model._components64[c]
        cb = ex.comp_bound[c]
        report("orthonormal", name, np.abs(V @ V.T - np.eye(V.shape[0])), cb[:, None] + cb[None, :] + np.outer(cb, cb))
    if name == "frac":
        assert ex.ratio_all[:ex.k].sum() > 0.9 >= ex.ratio_all[:ex.k - 1].sum()


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_transforms(cuda, name):
    ex = K.exact(name)
    model, T = fitted(name)
    c = ex.comparable
    assert T.is_cuda and T.dtype == torch.float32 and tuple(T.shape) == (ex.n, ex.k)
    want, bound = ex.transform(ex.X)
    T_h = T.cpu().numpy().astype(np.float64)
    report("fit_transform", name, np.abs(T_h - want)[:, c], bound[:, c])
    assert torch.equal(model.transform(ex.X), T)
    fresh = K.fresh_rows(name)
    want_f, bound_f = ex.transform(fresh)
    got_f = model.transform(torch.as_tensor(fresh)).cpu().numpy().astype(np.float64)
    report("transform", name, np.abs(got_f - want_f)[:, c], bound_f[:, c])
    if c.all():
        want_i, bound_i = ex.inverse(want, bound)
        got_i = model.inverse_transform(T).cpu().numpy().astype(np.float64)
        report("inverse_transform", name, np.abs(got_i - want_i), bound_i)
    with pytest.raises(ValueError):
        model.transform(np.zeros((3, ex.d + 1), np.float32))


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_triangle_against_sklearn(cuda, name):
    """|device - sklearn| <= |sklearn - exact| + bound: pins the sign rule and each attribute's definition."""
    ex = K.exact(name)
    fx = np.load(K.fixture_path(name))
    model, T = fitted(name)
    c = ex.comparable

    def tri(what, dev, sk, exact, bound):
        dev, sk = np.asarray(dev, np.float64), np.asarray(sk, np.float64)
        report("sk_" + what, name, np.abs(dev - sk), np.abs(sk - exact) + bound + K.half_spacing32(exact))

    tri("variance", model.explained_variance_, fx["explained_variance"], ex.variance, ex.variance_bound)
    tri("ratio", model.explained_variance_ratio_, fx["explained_variance_ratio"], ex.ratio, ex.ratio_bound)
    tri("singular", model.singular_values_, fx["singular_values"], ex.singular, ex.singular_bound)
    tri("noise", model.noise_variance_, fx["noise_variance"], ex.noise, ex.noise_bound)
    tri("mean", model.mean_, fx["mean"], ex.mean, ex.delta)
    tri("components", model.components_[c], fx["components"][c], ex.V[c], ex.comp_bound[c][:, None])
    rows = fx["transform"].shape[0]
    want, bound = ex.transform(ex.X[:rows])
    tri("transform", T[:rows].cpu().numpy()[:, c], fx["transform"][:, c], want[:, c], bound[:, c])


def test_constant_input_is_sklearns(cuda):
    import hlmc_amd
    fx = np.load(K.fixture_path(K.CONSTANT))
    model = hlmc_amd.PCA(3)
    T = model.fit_transform(K.case_input(K.CONSTANT))
    assert np.array_equal(model.components_, fx["components"]) and np.array_equal(model.mean_, fx["mean"])
    assert np.array_equal(model.explained_variance_, fx["explained_variance"])
    assert np.array_equal(model.singular_values_, fx["singular_values"])
    assert np.isnan(model.explained_variance_ratio_).all() and np.isnan(fx["explained_variance_ratio"]).all()
    assert float(model.noise_variance_) == float(fx["noise_variance"]) == 0.0
    assert np.array_equal(T.cpu().numpy(), fx["transform"])


@pytest.mark.parametrize("name,clusters", [("ref_simple", 6), ("ref_cvae", 5)])
def test_baseline(cuda, name, clusters):
    import hlmc_amd
    from hlmc_amd import metrics as M
    X = K.case_input(name)
    k = K.CASES[name]["k"]
    y = np.random.default_rng(3).integers(0, clusters, X.shape[0])
    feats, labels, scores = hlmc_amd.pca_kmeans_baseline(X, k, clusters, y_true=y, n_init=3)
    _, T = fitted(name)
    assert feats.is_cuda and torch.equal(feats, T)
    want = hlmc_amd.KMeans(n_clusters=clusters, random_state=42, n_init=3).fit_predict(T)
    assert np.array_equal(labels, want)
    assert scores == {"Silhouette": M.silhouette_score(T, want),
                      "Calinski-Harabasz": M.calinski_harabasz_score(T, want),
                      "NMI": M.normalized_mutual_info_score(y, want), "ARI": M.adjusted_rand_score(y, want),
                      "Purity": M.calculate_purity(y, want)}
    plain = hlmc_amd.pca_kmeans_baseline(X, k, clusters, n_init=3)[2]
    assert list(plain) == ["Silhouette", "Calinski-Harabasz"] and plain["Silhouette"] == scores["Silhouette"]
