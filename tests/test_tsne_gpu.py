"""GPU t-SNE against tests/tsne_check.py: each hlmc_tsne_* kernel inside its rounding bound of the exact reference at
the edge shapes (tile, block and slab boundaries, ties, duplicated rows, a full CSR row), bit-identical from run to run,
and whole fits held to the spread sklearn 1.7.2 shows between its own seeds (tests/golden/tsne_fits.npz).

Every comparison prints "TSNE_EOB <quantity> <worst |err| / bound>" before it asserts."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from sklearn.cluster import KMeans as SkKMeans
from sklearn.manifold import trustworthiness
from sklearn.metrics import adjusted_rand_score

import hlmc_amd
from hlmc_amd import _lib as L
from tests import tsne_check as K

pytestmark = pytest.mark.gpu


def report(quantity, err, bound):
    ratio = float(np.max(np.asarray(err, np.float64) / np.asarray(bound, np.float64)))
    print(f"TSNE_EOB {quantity} {ratio:.4f}")
    return ratio


def t(a, dev, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def dev_knn(dev, X, k):
    n, d = X.shape
    lib = L.lib()
    wsb = int(lib.hlmc_tsne_workspace(n, d, k))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    Xd = t(X, dev, np.float32)
    idx = torch.full((n, k), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((n, k), -1.0, dtype=torch.float64, device=dev)
    L.check(lib.hlmc_tsne_knn(L.stream(), Xd.data_ptr(), n, d, k, idx.data_ptr(), d2.data_ptr(), ws.data_ptr(), wsb))
    return idx.cpu().numpy(), d2.cpu().numpy()


def dev_affinities(dev, idx, d2, perp):
    n, k = idx.shape
    lib = L.lib()
    wsb = int(lib.hlmc_tsne_workspace(n, 1, k))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    idx_d, d2_d = t(idx, dev, np.int32), t(d2, dev, np.float64)
    beta = torch.empty(n, dtype=torch.float64, device=dev)
    cond = torch.empty(n, k, dtype=torch.float64, device=dev)
    indptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    indices = torch.full((2 * n * k,), -1, dtype=torch.int32, device=dev)
    values = torch.full((2 * n * k,), -1.0, dtype=torch.float32, device=dev)
    L.check(lib.hlmc_tsne_affinities(L.stream(), idx_d.data_ptr(), d2_d.data_ptr(), n, k, perp, beta.data_ptr(),
                                     cond.data_ptr(), indptr.data_ptr(), indices.data_ptr(), values.data_ptr(),
                                     ws.data_ptr(), wsb))
    ip = indptr.cpu().numpy()
    nnz = int(ip[-1])
    return beta.cpu().numpy(), cond.cpu().numpy(), ip, indices[:nnz].cpu().numpy(), values[:nnz].cpu().numpy()


class DevCsr:
    def __init__(self, dev, indptr, indices, values):
        self.n = len(indptr) - 1
        self.indptr, self.indices = t(indptr, dev, np.int64), t(indices, dev, np.int32)
        self.values = t(values, dev, np.float32)
        self.ws_bytes = int(L.lib().hlmc_tsne_workspace(self.n, 1, 1))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)


def dev_gradient(dev, csr, Y, exag, want_stats=1):
    Yd = t(Y, dev, np.float32)
    grad = torch.empty(csr.n, 2, dtype=torch.float32, device=dev)
    stats = torch.full((3,), -1.0, dtype=torch.float64, device=dev)
    L.check(L.lib().hlmc_tsne_gradient(L.stream(), Yd.data_ptr(), csr.n, csr.indptr.data_ptr(), csr.indices.data_ptr(),
                                       csr.values.data_ptr(), exag, grad.data_ptr(), stats.data_ptr(), want_stats,
                                       csr.ws.data_ptr(), csr.ws_bytes))
    return grad.cpu().numpy(), stats.cpu().numpy()


def dev_run(dev, csr, Y, update, gains, exag, momentum, lr, n_iter):
    Yd, ud, gd = t(Y, dev, np.float32).clone(), t(update, dev, np.float32).clone(), t(gains, dev, np.float32).clone()
    stats = torch.zeros(3, dtype=torch.float64, device=dev)
    L.check(L.lib().hlmc_tsne_run(L.stream(), Yd.data_ptr(), ud.data_ptr(), gd.data_ptr(), csr.n, csr.indptr.data_ptr(),
                                  csr.indices.data_ptr(), csr.values.data_ptr(), exag, momentum, lr, n_iter,
                                  stats.data_ptr(), csr.ws.data_ptr(), csr.ws_bytes))
    return Yd.cpu().numpy(), ud.cpu().numpy(), gd.cpu().numpy(), stats.cpu().numpy()


# ------------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize("name", list(K.KNN_CASES))
def test_knn(cuda, name):
    n, d, k, kind = K.KNN_CASES[name]
    X = K.knn_input(name)
    D, bound = K.sqdist_exact(X), K.sqdist_bound(X)
    want_idx, want_d = K.knn_from(D.astype(np.float64), k)
    idx, d2 = dev_knn(cuda, X, k)
    rows = np.arange(n)[:, None]
    assert ((idx >= 0) & (idx < n) & (idx != rows)).all()
    assert all(len(set(idx[i])) == k for i in range(n))
    report(f"knn_distance[{name}]", np.abs(d2 - D[rows, idx].astype(np.float64)), bound[rows, idx] + 1e-300)
    assert (np.abs(d2 - D[rows, idx].astype(np.float64)) <= bound[rows, idx]).all()
    # ascending by distance, equal distances by ascending index
    assert (np.diff(d2, axis=1) >= 0).all()
    tie = np.diff(d2, axis=1) == 0
    assert (np.diff(idx, axis=1)[tie] > 0).all()
    if kind == "dups":
        assert (np.abs(d2 - want_d) <= np.take_along_axis(bound, want_idx.astype(np.int64), 1).max()).all()
        same = np.r_[0, 2:22]                   # the 21 coincident rows: 20 neighbours at distance 0 each
        assert (d2[same] <= bound.max()).all() and tie.any()
    else:
        amb = K.knn_ambiguous_rows(D, bound, k)
        assert not amb.any()                 # the seeds leave no row undecided, so every row must agree
        bad = [i for i in range(n) if set(idx[i]) != set(want_idx[i])]
        assert not bad, bad[:5]
    idx2, d22 = dev_knn(cuda, X, k)
    assert np.array_equal(idx, idx2) and np.array_equal(d2, d22)


# ------------------------------------------------------------------------------------------------ affinities
@pytest.mark.parametrize("name", list(K.SEARCH_CASES))
def test_affinities(cuda, name):
    X, idx, d32, perp = K.search_input(name)
    n, k = idx.shape
    P_ref, beta_ref = K.search_reference(d32, perp)
    P_rs, beta_rs, border, steps = K.search_restated(d32, perp)
    assert border.sum() <= 0.01 * n
    beta, cond, indptr, indices, values = dev_affinities(cuda, idx, d32.astype(np.float64), perp)
    assert np.array_equal(beta[~border], beta_rs[~border]) and np.array_equal(beta_rs[~border], beta_ref[~border])
    if name == "wide":
        assert (beta < 1e-3).all()
    if name == "narrow":
        assert (beta > 1e3).all()
    H = K.perplexity_of(d32, beta)
    settled = steps < 100                    # a row whose neighbours are all equally far never settles (sklearn's too)
    assert (np.abs(H - np.log(perp))[settled] <= K.SEARCH_TOL * (1 + 1e-9)).all()
    assert settled.all() or name == "p5"
    if name == "p5":
        assert np.array_equal(cond[0], np.full(k, 1.0 / k))
    pb = K.cond_p_bound(P_ref, d32, beta_ref, k)
    report(f"cond_p[{name}]", np.abs(cond - P_ref)[~border], pb[~border])
    assert (np.abs(cond - P_ref)[~border] <= pb[~border]).all()
    ip, ix, want = K.joint_reference(idx, P_ref)
    assert np.array_equal(indptr, ip) and np.array_equal(indices, ix)
    if not border.any():
        vb = K.joint_value_bound(want, n, k)
        report(f"p_value[{name}]", np.abs(values.astype(np.float64) - want), vb)
        assert (np.abs(values.astype(np.float64) - want) <= vb).all()
    total_bound = 2 * K.V                    # every value is rounded once to float32: V of the values' sum
    report(f"p_total[{name}]", abs(float(values.astype(np.float64).sum()) - 1.0), total_bound)
    assert abs(float(values.astype(np.float64).sum()) - 1.0) <= total_bound
    Pm = sp.csr_matrix((values, indices, indptr), shape=(n, n)).toarray()
    assert np.array_equal(Pm, Pm.T)
    if name == "hub":
        assert indptr[1] - indptr[0] == n - 1
    again = dev_affinities(cuda, idx, d32.astype(np.float64), perp)
    assert all(np.array_equal(a, b) for a, b in zip((beta, cond, indptr, indices, values), again))


# ------------------------------------------------------------------------------------------------ gradient
GRAD_CASES = [(255, 1.0, 1.0, False), (256, 1e-4, 12.0, False), (257, 1.0, 12.0, False), (257, 50.0, 1.0, False),
              (513, 1e-4, 1.0, False), (513, 50.0, 12.0, False), (130, 1.0, 1.0, True), (130, 1e-4, 12.0, True)]


@pytest.mark.parametrize("n,scale,exag,hub", GRAD_CASES)
def test_gradient(cuda, n, scale, exag, hub):
    Y, indptr, indices, values = K.grad_case(n, scale, perp=5.0 if hub else 30.0, hub=hub)
    if hub:
        assert indptr[1] - indptr[0] == n - 1
    ref = K.GradRef(Y, indptr, indices, values, exag)
    csr = DevCsr(cuda, indptr, indices, values)
    grad, stats = dev_gradient(cuda, csr, Y, exag)
    tag = f"[n{n}_s{scale}_a{exag}{'_hub' if hub else ''}]"
    report("grad" + tag, np.abs(grad - ref.grad), ref.grad_bound)
    report("Z" + tag, abs(stats[0] - ref.Z), ref.Z_bound)
    report("KL" + tag, abs(stats[1] - ref.kl), ref.kl_bound)
    report("grad_norm" + tag, abs(stats[2] - ref.gnorm), ref.gnorm_bound)
    assert (np.abs(grad - ref.grad) <= ref.grad_bound).all()
    assert abs(stats[0] - ref.Z) <= ref.Z_bound
    assert abs(stats[1] - ref.kl) <= ref.kl_bound
    assert abs(stats[2] - ref.gnorm) <= ref.gnorm_bound
    # the slab partials of the documented workspace re-add to the result
    off = K.grad_workspace_offsets(n)
    S = off["slabs"]
    assert S == -(-n // 256)
    part = csr.ws[off["part"]:off["part"] + S * 3 * n * 8].view(torch.float64).cpu().numpy().reshape(S, 3, n)
    rep = K.combine_parts(part)
    assert K.block_sum_ordered(rep[2]) == stats[0]
    want_part = K.repulsion_restated(Y)
    q_abs = np.stack([ref.rep_abs[:, 0], ref.rep_abs[:, 1], ref.Z_bound / K.Z_V * np.ones(n)])   # loose per slab
    assert (np.abs(part - want_part) <= (K.REP_V + n * K.U) * q_abs[None] + 1e-300).all()
    z = max(stats[0], K.EPS64)
    regrad = 4.0 * (ref.attr - rep[:2].T / z)
    rb = K.half_spacing32(regrad) * (1 + 1e-6) + 4.0 * (np.diff(indptr)[:, None] + 8) * K.U * ref.attr_abs \
        + 16 * K.U * np.abs(rep[:2].T) / z
    report("grad_from_parts" + tag, np.abs(grad - regrad), rb)
    assert (np.abs(grad - regrad) <= rb).all()
    # without the statistics the gradient and Z are the same bits; two runs are bit-identical
    g0, s0 = dev_gradient(cuda, csr, Y, exag, want_stats=0)
    assert np.array_equal(g0, grad) and s0[0] == stats[0] and s0[1] == -1.0
    g2, s2 = dev_gradient(cuda, csr, Y, exag)
    assert np.array_equal(g2, grad) and np.array_equal(s2, stats)


# ------------------------------------------------------------------------------------------------ update step
@pytest.mark.parametrize("exag,momentum,lr", [(12.0, 0.5, 50.0), (1.0, 0.8, 200.0)])
def test_update_step(cuda, exag, momentum, lr):
    n = 257
    Y, indptr, indices, values = K.grad_case(n, 1.0)
    rng = np.random.default_rng(11)
    update = rng.normal(0.0, 1e-2, (n, 2)).astype(np.float32)
    gains = rng.choice(np.array([0.01, 0.0125, 0.8, 1.0, 1.2, 2.6], np.float32), (n, 2))
    ref = K.GradRef(Y, indptr, indices, values, exag)
    csr = DevCsr(cuda, indptr, indices, values)
    Y1, u1, g1, stats = dev_run(cuda, csr, Y, update, gains, exag, momentum, lr, 1)
    pw, uw, gw = K.gradient_descent_step(Y, update, gains, ref.grad.astype(np.float32), momentum, lr)
    decided = np.abs(ref.grad) > ref.grad_bound          # elsewhere the sign of update * grad may differ
    assert decided.mean() > 0.99
    assert np.array_equal(g1[decided], gw[decided])
    assert (g1 >= np.float32(0.01)).all() and (g1 == np.float32(0.01)).any()
    ub, pb = K.update_bounds(update, gw.astype(np.float64), ref.grad, ref.grad_bound, momentum, lr)
    report(f"update[a{exag}]", np.abs(u1 - uw.astype(np.float64))[decided], ub[decided])
    report(f"Y_step[a{exag}]", np.abs(Y1 - pw.astype(np.float64))[decided], pb[decided])
    assert (np.abs(u1 - uw.astype(np.float64))[decided] <= ub[decided]).all()
    assert (np.abs(Y1 - pw.astype(np.float64))[decided] <= pb[decided]).all()
    assert abs(stats[1] - ref.kl) <= ref.kl_bound and abs(stats[2] - ref.gnorm) <= ref.gnorm_bound
    # hlmc_tsne_run(n_iter=3) is three single iterations, bit for bit
    Y3, u3, g3, s3 = dev_run(cuda, csr, Y, update, gains, exag, momentum, lr, 3)
    Ys, us, gs = Y, update, gains
    for _ in range(3):
        Ys, us, gs, ss = dev_run(cuda, csr, Ys, us, gs, exag, momentum, lr, 1)
    assert np.array_equal(Y3, Ys) and np.array_equal(u3, us) and np.array_equal(g3, gs) and np.array_equal(s3, ss)


# ------------------------------------------------------------------------------------------------ whole fits
def ari_of(Y, y, centres):
    return adjusted_rand_score(y, SkKMeans(centres, n_init=10, random_state=0).fit_predict(Y))


@pytest.mark.parametrize("name", list(K.FIT_CASES))
def test_fit_is_inside_sklearns_own_spread(cuda, name):
    c = K.FIT_CASES[name]
    X, y = K.fit_input(name)
    fx = K.fit_fixture()
    assert str(fx["sklearn_version"]) == "1.7.2"
    m = hlmc_amd.TSNE(n_components=2, perplexity=c["perplexity"], random_state=42, device=cuda)
    out = m.fit_transform(X)
    assert out.is_cuda and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), m.embedding_)
    assert m.embedding_.shape == (c["n"], 2) and m.embedding_.dtype == np.float32 and np.isfinite(m.embedding_).all()
    assert m.n_iter_ == 999 and m.n_features_in_ == c["d"]
    assert m.learning_rate_ == float(fx[f"{name}_learning_rate"])
    assert ari_of(m.embedding_, y, c["centres"]) == 1.0
    indptr, indices, values = m.affinities_.csr()
    kl = K.exact_kl(indptr, indices, values, m.embedding_)
    trust = trustworthiness(X, m.embedding_, n_neighbors=5)
    kls, trs = fx[f"{name}_kl_exact"], fx[f"{name}_trustworthiness"]
    kl_max = kls.max() + (kls.max() - kls.min())
    tr_min = trs.min() - (trs.max() - trs.min())
    print(f"TSNE_FIT {name} KL {kl:.6f} (sklearn {kls.min():.6f}..{kls.max():.6f}, limit {kl_max:.6f}) "
          f"trust {trust:.6f} (sklearn {trs.min():.6f}..{trs.max():.6f}, limit {tr_min:.6f})")
    assert kl <= kl_max
    assert trust >= tr_min
    # kl_divergence_ is the error of the last iteration, taken (as in sklearn) before that iteration's update
    ref = K.GradRef(m._kl_embedding, indptr, indices, values, 1.0)
    report(f"kl_divergence_[{name}]", abs(m.kl_divergence_ - ref.kl), ref.kl_bound)
    assert abs(m.kl_divergence_ - ref.kl) <= ref.kl_bound


def test_two_fits_are_bit_identical_and_other_inits(cuda):
    name = "n300_d16"
    c = K.FIT_CASES[name]
    X, y = K.fit_input(name)
    a = hlmc_amd.TSNE(perplexity=c["perplexity"], device=cuda).fit(X)
    b = hlmc_amd.TSNE(perplexity=c["perplexity"], device=cuda).fit(torch.as_tensor(X, device=cuda))
    assert np.array_equal(a.embedding_, b.embedding_) and a.kl_divergence_ == b.kl_divergence_
    r = hlmc_amd.TSNE(perplexity=c["perplexity"], init="random", random_state=3, device=cuda).fit(X)
    assert r.n_iter_ == 999 and ari_of(r.embedding_, y, c["centres"]) == 1.0
    r2 = hlmc_amd.TSNE(perplexity=c["perplexity"], init="random", random_state=3, device=cuda).fit(X)
    assert np.array_equal(r.embedding_, r2.embedding_) and not np.array_equal(r.embedding_, a.embedding_)
    Y0 = (1e-4 * np.random.RandomState(5).standard_normal((c["n"], 2))).astype(np.float32)
    g = hlmc_amd.TSNE(perplexity=c["perplexity"], init=Y0, device=cuda).fit(X)
    assert g.n_iter_ == 999 and ari_of(g.embedding_, y, c["centres"]) == 1.0
