"""Op-level parity of the restart-batched k-means kernels (csrc/kmeans.hip), called through hlmc_amd._lib, against
the numpy restatements of sklearn in oracle/kmeans_oracle.py -- at odd feature counts, d < 32, holes in the `active`
mask up to bit 63, per-restart offsets (labels + r n, centres + r k d, prev + (r prevT + best[r]) n) and R x T up to
64 -- and whole KMeans fits off the workload's shapes (more than one lockstep group, the LDS-capped group size, k up
to 55, an input whose empty clusters are relocated) against the oracle's KMeans, which tests/test_oracle_cpu.py pins
to live sklearn on the same inputs.

Every output buffer is pre-filled with a sentinel (NaN / 0x7f7f7f7f) and carries one spare row, so "written",
"left untouched" and "wrote past the end" are all observable.  Labels are always in [0, k) and candidate rows in
[0, n): the kernels index with them unchecked."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import kmeans_oracle as KO
from tests import kmeans_cases as KC

pytestmark = pytest.mark.gpu

SENT = 0x7F7F7F7F


def _dev(a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")     # a copy: the cached references are read-only


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda")


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _assert_bits_equal(got, want, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# ------------------------------------------------------------------ float64 candidate distances
CAND16 = [0, 5, 2, KC.SQDIST_N - 1, 3, 1, 7, 64, 65, 128, 200, 255, 256, 257, 300, KC.SQDIST_N - 2]
assert CAND16[:5] == KC.SQDIST_CAND


@functools.lru_cache(maxsize=None)
def _sqdist_reference(d):
    """(X, exact, bound, sklearn's upcast restatement) for the 16 candidates; computed once per d, read-only."""
    X = KC.dup_rows(KC.SQDIST_N, d, seed=d)
    A = X[CAND16]
    out = (X, KO.sqdist_exact(A, X), KO.sqdist_bound(A, X, d), KO._sqdist_upcast(A, X))
    for a in out:
        a.setflags(write=False)
    return out


def _sqdist_rows(Xd, cand):
    n, d = Xd.shape
    out = _nan(len(cand) + 1, n)
    L.check(L.lib().hlmc_km_sqdist_rows(L.stream(), Xd.data_ptr(), n, d, L.i64_array(cand), len(cand), out.data_ptr()),
            "hlmc_km_sqdist_rows")
    return _host(out)


def _pp_dist(Xd, cand, R, T, prev=None, prevT=1, best=None):
    n, d = Xd.shape
    out = _nan(R * T + 1, n)
    cd = _dev(np.asarray(cand, np.int64))
    L.check(L.lib().hlmc_km_pp_dist(L.stream(), Xd.data_ptr(), n, d, R, T, cd.data_ptr(),
                                    None if prev is None else prev.data_ptr(), prevT,
                                    None if best is None else _i32p(best), out.data_ptr()), "hlmc_km_pp_dist")
    return _host(out)


@pytest.mark.parametrize("ncand", [1, 5, 16])
@pytest.mark.parametrize("d", [1, 3, 8, 12, 37, 130])
def test_km_sqdist_rows_and_pp_dist_within_bound_of_exact(cuda, d, ncand):
    """hlmc_km_sqdist_rows and hlmc_km_pp_dist (prev = NULL): float32(max(0, float64 (-2 a.x + ||a||^2) + ||x||^2))
    within oracle sqdist_bound (half a float32 ulp + the float64 summation bound, derived) of the exact squared
    distance, through einsum_sq_f64's 8-block (d >= 8), pair tail and odd tail; a candidate's own row and its exact
    duplicate clip to <= the bound; and the two kernels agree bit for bit, as include/hlmc.h promises."""
    X, exact, bound, upcast = _sqdist_reference(d)
    n = X.shape[0]
    cand = CAND16[:ncand]
    Xd = _dev(X)
    rows = _sqdist_rows(Xd, cand)
    pp = _pp_dist(Xd, cand, ncand, 1)
    for what, got in (("sqdist_rows", rows), ("pp_dist", pp)):
        assert np.isnan(got[ncand]).all(), f"{what} wrote past its last row"
        got = got[:ncand]
        assert not np.isnan(got).any(), f"{what} left elements unwritten"
        err = np.abs(got.astype(np.float64) - exact[:ncand])
        flips = int((_bits(got) != _bits(upcast[:ncand])).sum())
        print(f"{what} d={d} ncand={ncand}: worst err / bound {float((err / bound[:ncand]).max()):.3f}, "
              f"{flips} of {got.size} elements not bit-equal to _sqdist_upcast")
        assert (err <= bound[:ncand]).all(), what
        for t, c in enumerate(cand):
            assert 0.0 <= got[t, c] <= bound[t, c], (what, t, c, got[t, c])
        assert 0.0 <= got[0, 1] <= bound[0, 1], what                  # row 1 is an exact copy of candidate row 0
    _assert_bits_equal(pp[:ncand], rows[:ncand], "pp_dist != sqdist_rows")


@pytest.mark.parametrize("R,T,prevT", [(3, 5, 5), (12, 5, 1), (64, 1, 3), (1, 64, 2)])
def test_km_pp_dist_running_minimum_per_restart(cuda, R, T, prevT):
    """hlmc_km_pp_dist with prev: out[r][t] = min(prev[r][best[r]], dist(X[cand[r][t]], .)) with best differing per
    restart (prevT - 1 included) and R x T in {15, 60, 64, 64} (not a multiple of the kernel's 8-candidate pass; the
    limit).  The distance is the prev = NULL launch's (checked against the exact value); the minimum is exact."""
    n, d = 300, 12
    X = KC.dup_rows(n, d, seed=R * 100 + T)
    rng = np.random.default_rng(R * 1000 + T * 10 + prevT)
    cand = rng.integers(0, n, R * T)
    cand[:4] = [0, n - 1, 2, 3][:min(4, R * T)]
    # every prev row is different, so a read of another restart's or another trial's row shows; ~ half the elements
    # lie below the distances (~ 2 d 3^2)
    prev = rng.uniform(0.0, 4.0 * d * 9.0, (R, prevT, n)).astype(np.float32)
    best = ((prevT - 1 - np.arange(R)) % prevT).astype(np.int32)
    assert best[0] == prevT - 1 and (prevT == 1 or R == 1 or len(set(best.tolist())) > 1)
    Xd = _dev(X)
    dist = _pp_dist(Xd, cand, R, T)[:R * T]
    exact, bound = KO.sqdist_exact(X[cand], X), KO.sqdist_bound(X[cand], X, d)
    err = np.abs(dist.astype(np.float64) - exact)
    print(f"pp_dist R={R} T={T}: worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    got = _pp_dist(Xd, cand, R, T, prev=_dev(prev), prevT=prevT, best=best)
    assert np.isnan(got[R * T]).all() and not np.isnan(got[:R * T]).any()
    got = got[:R * T]
    closest = np.repeat(prev[np.arange(R), best], T, axis=0)           # [R*T][n]: restart rt // T's own row
    from_prev, from_dist = _bits(got) == _bits(closest), _bits(got) == _bits(dist)
    assert (from_prev | from_dist).all()
    _assert_bits_equal(got, np.minimum(closest, dist))
    assert 0.2 < from_prev.mean() < 0.8, "the inputs no longer exercise both sides of the minimum"


def test_km_pp_search_per_restart_rows(cuda):
    """hlmc_km_pp_search with R = 3, T = 4, prevT = 3 and a different best row per restart: every decided draw equals
    np.searchsorted(np.cumsum(row, float64), rv) of that restart's own row prev[r][best[r]]; the draws placed exactly
    on a prefix are flagged, the midpoints are decided."""
    R, T, prevT, n = 3, 4, 3, 1000
    rng = np.random.default_rng(17)
    prev = (rng.random((R, prevT, n)) * (1.0 + np.arange(R * prevT).reshape(R, prevT, 1))).astype(np.float32)
    best = np.array([2, 0, 1], dtype=np.int32)
    rv = np.empty((R, T), np.float64)
    ref = np.empty((R, T), np.int64)
    for r in range(R):
        cs = np.cumsum(prev[r, best[r]], dtype=np.float64)
        i0, i1 = 37 + 200 * r, 959 + r                                 # i1: the last wave's 64-row segment
        rv[r] = [0.5 * (cs[i0] + cs[i0 + 1]), 0.25 * cs[0] if r == 1 else 0.5 * (cs[500 + r] + cs[501 + r]),
                 0.5 * (cs[i1] + cs[i1 + 1]), cs[300 + 64 * r]]
        ref[r] = np.minimum(np.searchsorted(cs, rv[r]), n - 1)
        # the same draws in another of this restart's rows give other answers: a wrong offset cannot pass
        other = np.cumsum(prev[r, (best[r] + 1) % prevT], dtype=np.float64)
        assert (np.searchsorted(other, rv[r]) != ref[r]).sum() >= 3
    cand = torch.full((R * T + 1,), -1, dtype=torch.int64, device="cuda")
    amb = _sent(R * T + 1)
    pd = _dev(prev)
    L.check(L.lib().hlmc_km_pp_search(L.stream(), n, R, T, pd.data_ptr(), prevT, _i32p(best),
                                      np.ascontiguousarray(rv).ctypes.data_as(C.POINTER(C.c_double)),
                                      cand.data_ptr(), amb.data_ptr()), "hlmc_km_pp_search")
    cand, amb = _host(cand), _host(amb)
    assert cand[R * T] == -1 and amb[R * T] == SENT
    cand, amb = cand[:R * T].reshape(R, T), amb[:R * T].reshape(R, T)
    print(f"pp_search amb {amb.tolist()}, candidates {cand.tolist()} vs numpy {ref.tolist()}")
    assert set(np.unique(amb).tolist()) <= {0, 1}
    assert amb[:, 3].all(), "a draw exactly on a cumsum prefix must be flagged"
    assert not amb[:, :3].any(), "a draw midway between two prefixes must be decided"
    np.testing.assert_array_equal(cand[amb == 0], ref[amb == 0])


# ------------------------------------------------------------------ E-step
def _near_tie_problem(n, d, k, R, seed):
    """The near-tie construction of test_km_assign_matches_sklearn_estep with one centre set per restart: the rows
    lie within 1e-6 of the bisector of two centres; every restart keeps that pair (at its own two indices, so the
    tie is between other labels) and draws its other centres afresh."""
    rng = np.random.default_rng(seed)
    pair = rng.standard_normal((2, d)).astype(np.float32)
    t = rng.standard_normal((n, d)).astype(np.float32)
    m, u = (pair[0] + pair[1]) / 2, pair[1] - pair[0]
    u = u / np.linalg.norm(u)
    t = t - np.outer(t @ u, u)
    X = (m + 0.3 * t + np.outer(rng.standard_normal(n) * 1e-6, u)).astype(np.float32)
    Cs = rng.standard_normal((R, k, d)).astype(np.float32)
    for r in range(R):
        at = rng.permutation(k)[:2]
        Cs[r, at[0]], Cs[r, at[1]] = pair[0], pair[1]
    return X, Cs


@pytest.mark.parametrize("n,d,k,R,active", [
    (515, 33, 4, 5, 0b10110),          # small-matrix path, last chunk of 3 rows, a hole in the mask
    (515, 33, 5, 2, 0b11),             # k % 4 = 1: the small path's halves-first tree in the 3-row last chunk
    (300, 20, 7, 3, 0b111),            # d < 32: never the small-matrix path
    (130, 5, 3, 64, (1 << 63) | 1),    # R = 64, only bits 63 and 0
    (1000, 130, 17, 2, 0b01),          # k > 16 (two passes of the 4-cluster interleave), d % 16 = 2
], ids=lambda v: str(v))
def test_km_assign_batch_mask_offsets_and_counts(cuda, n, d, k, R, active):
    """hlmc_km_assign_batch: labels of active restarts equal the oracle's E-step (KO.assign_labels) per restart;
    restarts outside the mask keep the sentinel; n_changed[r] += count(labels != labels_old) for active restarts
    only (it starts at 7); with labels_old = NULL n_changed is not touched."""
    X, Cs = _near_tie_problem(n, d, k, R, seed=n * 31 + d * 7 + k)
    act = [r for r in range(R) if (active >> r) & 1]
    ref = {r: KO.assign_labels(X, Cs[r]) for r in act}
    rng = np.random.default_rng(R + n)
    old = rng.integers(0, k, (R, n)).astype(np.int32)
    for r in act:
        keep = rng.random(n) < 0.7
        old[r, keep] = ref[r][keep]
    Xd, Cd, oldd = _dev(X), _dev(Cs), _dev(old)
    for with_old in (True, False):
        lab = _sent(R + 1, n)
        chg = torch.full((R + 1,), 7, dtype=torch.int32, device="cuda")
        L.check(L.lib().hlmc_km_assign_batch(L.stream(), Xd.data_ptr(), n, d, Cd.data_ptr(), k, R, active,
                                             lab.data_ptr(), oldd.data_ptr() if with_old else None, chg.data_ptr()),
                "hlmc_km_assign_batch")
        lab, chg = _host(lab), _host(chg)
        assert (lab[R] == SENT).all() and chg[R] == 7
        for r in range(R):
            if r in ref:
                np.testing.assert_array_equal(lab[r], ref[r], err_msg=f"restart {r}")
                want = 7 + (int((old[r] != ref[r]).sum()) if with_old else 0)
            else:
                assert (lab[r] == SENT).all(), f"inactive restart {r} was written"
                want = 7
            assert chg[r] == want, (r, with_old, int(chg[r]), want)


# ------------------------------------------------------------------ M-step
@pytest.mark.parametrize("k", [1, 5, 70])
@pytest.mark.parametrize("d", [3, 65])
@pytest.mark.parametrize("n", [700, 4096, 4097])
def test_km_sums_batch_row_order_bitexact_per_restart(cuda, n, d, k):
    """hlmc_km_sums_batch, R = 3 with restart 1 masked out: sums and weights equal sklearn's single-thread row-order
    float32 sums (KO.cluster_sums_f32) bit for bit per restart -- n = 4097 takes the partition path with one row in
    its last tile, n <= 4096 the one-launch path; a heavy cluster and (k > 1) empty clusters in every restart."""
    R, active = 3, 0b101
    rng = np.random.default_rng(n + d + k)
    X = rng.normal(0, 2.0, (n, d)).astype(np.float32)
    lab = rng.integers(0, k, (R, n)).astype(np.int32)
    for r in range(R):
        heavy = r % k
        lab[r, : n // 3] = heavy
        if k > 1:
            lab[r][lab[r] == (heavy + 1 + r) % k] = heavy              # one cluster left empty, another per restart
        if k == 70:
            lab[r][lab[r] % 3 == 1] = heavy                            # and a third of them
        assert k == 1 or (np.bincount(lab[r], minlength=k) == 0).any()
    Xd, ld = _dev(X), _dev(lab)
    sums, w = _nan(R + 1, k, d), _nan(R + 1, k)
    nb = int(L.lib().hlmc_km_sums_workspace(n, k)) * R
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    L.check(L.lib().hlmc_km_sums_batch(L.stream(), Xd.data_ptr(), n, d, ld.data_ptr(), k, R, active, sums.data_ptr(),
                                       w.data_ptr(), ws.data_ptr(), nb), "hlmc_km_sums_batch")
    sums, w = _host(sums), _host(w)
    assert np.isnan(sums[R]).all() and np.isnan(w[R]).all()
    for r in range(R):
        if (active >> r) & 1:
            rs, rw = KO.cluster_sums_f32(X, lab[r], k)
            _assert_bits_equal(sums[r], rs, f"sums of restart {r}")
            _assert_bits_equal(w[r], rw, f"weights of restart {r}")
        else:
            assert np.isnan(sums[r]).all() and np.isnan(w[r]).all(), f"inactive restart {r} was written"


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("d", [3, 8, 130])
def test_km_update_batch_centres_shifts_and_empty_flag(cuda, d, k):
    """hlmc_km_update_batch, R = 4 with restart 2 masked out and one zero weight in restart 1:
    C_new = sums * float32(1.0 / w) and info[:k] = the centre shifts in _euclidean_dense_dense order, bit for bit,
    info[k] = 0; the restart with the empty cluster writes info[k] = 1 and nothing else; the masked one nothing."""
    R, active = 4, 0b1011
    rng = np.random.default_rng(d * 10 + k)
    sums = rng.normal(0, 30.0, (R, k, d)).astype(np.float32)
    w = rng.integers(1, 50, (R, k)).astype(np.float32)
    w[1, k - 1] = 0.0
    C_old = rng.normal(0, 2.0, (R, k, d)).astype(np.float32)
    C_new, info = _nan(R + 1, k, d), _nan(R + 1, k + 1)
    sd, wd, od = _dev(sums), _dev(w), _dev(C_old)
    L.check(L.lib().hlmc_km_update_batch(L.stream(), k, d, R, active, sd.data_ptr(), wd.data_ptr(), od.data_ptr(),
                                         C_new.data_ptr(), info.data_ptr()), "hlmc_km_update_batch")
    C_new, info = _host(C_new), _host(info)
    assert np.isnan(C_new[R]).all() and np.isnan(info[R]).all()
    for r in (0, 3):
        ref = np.stack([sums[r, j] * np.float32(1.0 / float(w[r, j])) for j in range(k)])
        assert ref.dtype == np.float32
        _assert_bits_equal(C_new[r], ref, f"centres of restart {r}")
        _assert_bits_equal(info[r, :k], KO.euclidean_dense_dense_sq(ref, C_old[r]), f"shifts of restart {r}")
        assert info[r, k] == 0.0
    assert info[1, k] == 1.0 and np.isnan(info[1, :k]).all() and np.isnan(C_new[1]).all()
    assert np.isnan(info[2]).all() and np.isnan(C_new[2]).all()


# ------------------------------------------------------------------ row distances and inertia
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 2500])
@pytest.mark.parametrize("d", [1, 3, 4, 37, 130])
def test_km_rowdist_and_inertia_bitexact(cuda, d, n):
    """hlmc_km_rowdist / hlmc_km_inertia (R = 1) and hlmc_km_inertia_batch (R = 1, 3): row distances equal sklearn's
    _euclidean_dense_dense (KO.euclidean_dense_dense_sq: 4-element groups, then the d % 4 tail) and the inertia its
    sequential float32 sum (KO.inertia_f32), bit for bit, per restart with its own centres and labels -- n = 1, less
    than one 1024-value round of the sequential sum, exactly one, one more, several."""
    k, R = 6, 3
    rng = np.random.default_rng(d * 10000 + n)
    X = rng.normal(0.5, 2.0, (n, d)).astype(np.float32)
    Cs = rng.normal(0.5, 2.0, (R, k, d)).astype(np.float32)
    lab = rng.integers(0, k, (R, n)).astype(np.int32)
    for r in range(R):
        m = min(n, k)
        lab[r, :m] = ((np.arange(m) + r) % k)[::-1] if n >= k else k - 1   # every cluster used; n = 1: the last one
    rows = np.stack([KO.euclidean_dense_dense_sq(X, Cs[r][lab[r]]) for r in range(R)])
    inert = [KO.inertia_f32(X, Cs[r], lab[r]) for r in range(R)]
    lib = L.lib()
    Xd, Cd, ld = _dev(X), _dev(Cs), _dev(lab)
    out = _nan(n + 1)
    L.check(lib.hlmc_km_rowdist(L.stream(), Xd.data_ptr(), n, d, Cd.data_ptr(), ld.data_ptr(), out.data_ptr()),
            "hlmc_km_rowdist")
    out = _host(out)
    assert np.isnan(out[n])
    _assert_bits_equal(out[:n], rows[0], "hlmc_km_rowdist")
    one, tmp = _nan(2), _nan(n + 1)
    L.check(lib.hlmc_km_inertia(L.stream(), Xd.data_ptr(), n, d, Cd.data_ptr(), ld.data_ptr(), one.data_ptr(),
                                tmp.data_ptr()), "hlmc_km_inertia")
    one, tmp = _host(one), _host(tmp)
    assert np.isnan(one[1]) and np.isnan(tmp[n])
    _assert_bits_equal(tmp[:n], rows[0], "hlmc_km_inertia row distances")
    assert float(one[0]) == inert[0]
    for Rb in (1, 3):
        res, tmp = _nan(Rb + 1), _nan(Rb + 1, n)
        L.check(lib.hlmc_km_inertia_batch(L.stream(), Xd.data_ptr(), n, d, Cd.data_ptr(), k, ld.data_ptr(), Rb,
                                          res.data_ptr(), tmp.data_ptr()), "hlmc_km_inertia_batch")
        res, tmp = _host(res), _host(tmp)
        assert np.isnan(res[Rb]) and np.isnan(tmp[Rb]).all()
        _assert_bits_equal(tmp[:Rb], rows[:Rb], f"hlmc_km_inertia_batch R={Rb} row distances")
        assert [float(v) for v in res[:Rb]] == inert[:Rb], Rb


# ------------------------------------------------------------------ whole fits off the workload's shapes
@pytest.mark.parametrize("case", KC.FIT_CASES, ids=KC.FIT_IDS)
def test_kmeans_fit_matches_oracle_off_workload_shapes(cuda, case, monkeypatch):
    """hlmc_amd.KMeans against the oracle's KMeans (pinned to live sklearn on these inputs on the CPU): labels,
    inertia and n_iter equal, centres within float32 rounding, predict(X) == labels_; the lockstep restart groups
    that ran are the ones the case is there for (a second group; the LDS-capped size 15 at d = 400)."""
    name, kind, n, d, true_k, k, n_init = case
    X = KC.fit_input(case)
    zero_weight_calls = []
    sums_f32 = KO.cluster_sums_f32

    def counting_sums(Xc, labels, kk):
        s, w = sums_f32(Xc, labels, kk)
        zero_weight_calls.append(bool((w == 0).any()))
        return s, w

    monkeypatch.setattr(KO, "cluster_sums_f32", counting_sums)
    ref = KO.KMeans(k, random_state=42, n_init=n_init).fit(X)
    monkeypatch.setattr(KO, "cluster_sums_f32", sums_f32)
    if case == KC.RELOCATION_CASE:
        assert sum(zero_weight_calls) > 0, "the oracle relocated no empty cluster: the case is vacuous"
    groups = []
    pp = hlmc_amd.KMeans._kmeans_plusplus_batch

    def spy(self, Xc, seeds, trials):
        groups.append(len(seeds))
        return pp(self, Xc, seeds, trials)

    monkeypatch.setattr(hlmc_amd.KMeans, "_kmeans_plusplus_batch", spy)
    km = hlmc_amd.KMeans(n_clusters=k, random_state=42, n_init=n_init).fit(X)
    print(f"{name}: restart groups {groups}, n_iter {km.n_iter_}, oracle M-steps with an empty cluster "
          f"{sum(zero_weight_calls)}")
    assert groups == KC.fit_groups(case)
    np.testing.assert_array_equal(km.labels_, ref.labels_)
    assert km.inertia_ == ref.inertia_
    assert km.n_iter_ == ref.n_iter_
    np.testing.assert_allclose(km.cluster_centers_, ref.cluster_centers_, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(km.predict(X), km.labels_)
