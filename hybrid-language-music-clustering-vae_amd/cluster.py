"""KMeans (sklearn semantics) with the distance / assign / update work on the GPU.

Replaces ``sklearn.cluster.KMeans(n_clusters=k, random_state=42, n_init=10).fit_predict`` at
src/Convolutional_VAE.py:317-319,379-380, src/Conditional_VAE.py:293-295 (and the n_init='auto'
call at :528), src/Simple_VAE.py:244-261.

The n_init restarts run in lockstep on the device (round 5): every stage is one launch for all of them.
sklearn draws every restart's random numbers from one RandomState stream in a data-independent amount
(``seeding_draws``), so they are drawn up front in sklearn's order.  Device kernels (libhlmc) compute the
numpy-order column mean/variance, the k-means++ candidate draw (searchsorted of the float64 cumsum, exact
through an error bracket with a numpy fallback for undecidable draws), the float64-upcast candidate distances
and their running minimum, the float32 E-step (||c||^2 - 2 x.c, first minimum) in the exact rounding order of
sklearn's einsum row norms and its OpenBLAS sgemm call (oracle/kmeans_oracle.py estep_dist), per-cluster sums in
sklearn's single-thread row order, the centre update (float32 ``*= 1/w``) with its shifts, and inertia.  The
host keeps what sklearn's order depends on BLAS for or decides per restart: the float32 potentials (BLAS dot
products of the copied-back distances), the candidate argmin, empty-cluster relocation, the strict / tolerance
convergence tests and the best-of-n_init rule with ``_is_same_clustering``; one copy back per k-means++ step
and per Lloyd iteration serves all restarts.

Multi-GPU (``process_group=``): the n_init restarts are independent objects, so they shard across ranks
with no collective on the data path.  Every rank holds the same (small, [N, D] f32) latents and runs the
k-means++ seeding and Lloyd iterations of restarts ``i % world == rank`` only.  sklearn draws every restart's
seeds from one RandomState stream; a seeding consumes a data-independent number of doubles
(``seeding_draws``), so a rank skips another rank's seeding by drawing and discarding exactly that many and
its own restarts see the same random numbers as in a single process.  One ``all_gather_object`` of (restart,
labels, inertia, centres, n_iter) at the end feeds sklearn's sequential best-of rule in restart order, so the
result is bit-identical for any world size.

kmeans_k_sweep (after KMeans) is the k = 2..14 search of src/Convolutional_VAE.py:311-329 and src/Simple_VAE.py:244-251:
X is uploaded and centred once, and the silhouettes of all k come from one metrics.silhouette_scores call.

DBSCAN (end of this file) replaces ``sklearn.cluster.DBSCAN(eps, min_samples=5).fit_predict`` and the eps search at
src/Convolutional_VAE.py:347-374,382: fp64 MFMA neighbourhoods and union-find labelling on the device.

AgglomerativeClustering (after DBSCAN) replaces ``sklearn.cluster.AgglomerativeClustering(n_clusters=k).fit_predict``
and the k sweep at src/Convolutional_VAE.py:334-342,381: scipy's float64 distances and the nearest-neighbour chain with
the Ward update on the device, sort / relabel / cut of the n - 1 merge records on the host.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L


def _is_same_clustering(a, b, k):
    mapping = np.full(k, -1, dtype=np.int64)
    for x, y in zip(a, b):
        if mapping[x] == -1:
            mapping[x] = y
        elif mapping[x] != y:
            return False
    return True


def _euclid_f32(a, b):
    """sklearn _euclidean_dense_dense (float32, 4-element groups, no FMA) for each row pair."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    d = a.shape[-1]
    q = d // 4
    r = np.zeros(a.shape[:-1], np.float32)
    for g in range(q):
        s = (a[..., 4 * g] - b[..., 4 * g]) * (a[..., 4 * g] - b[..., 4 * g])
        s = s + (a[..., 4 * g + 1] - b[..., 4 * g + 1]) * (a[..., 4 * g + 1] - b[..., 4 * g + 1])
        s = s + (a[..., 4 * g + 2] - b[..., 4 * g + 2]) * (a[..., 4 * g + 2] - b[..., 4 * g + 2])
        s = s + (a[..., 4 * g + 3] - b[..., 4 * g + 3]) * (a[..., 4 * g + 3] - b[..., 4 * g + 3])
        r = r + s
    for c in range(4 * q, d):
        r = r + (a[..., c] - b[..., c]) * (a[..., c] - b[..., c])
    return r


def _pinned_like(t):
    return torch.empty(t.shape, dtype=t.dtype).pin_memory()


def _copy_back(dev, pairs):
    """The one copy back of a k-means++ step / Lloyd iteration: asynchronous copies into preallocated pinned host
    images ((pinned, device) pairs), one stream synchronisation, numpy views (valid until the image is reused)."""
    for pin, src in pairs:
        pin.copy_(src, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return [pin.numpy() for pin, _ in pairs]


class KMeans:
    def __init__(self, n_clusters=8, *, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, verbose=0,
                 random_state=None, copy_x=True, algorithm="lloyd", device=None, process_group=None):
        if init != "k-means++" or algorithm not in ("lloyd", "auto"):
            raise ValueError("only init='k-means++', algorithm='lloyd' are implemented (the reference's defaults)")
        self.n_clusters, self.init, self.n_init, self.max_iter, self.tol = n_clusters, init, n_init, max_iter, tol
        self.verbose, self.random_state, self.copy_x, self.algorithm = verbose, random_state, copy_x, algorithm
        self.device = device
        self.process_group = process_group

    # ------------------------------------------------------------------ device helpers
    def _dev(self):
        return torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    def _center(self, Xd):
        n, d = Xd.shape
        mean = torch.empty(d, dtype=torch.float32, device=Xd.device)
        var = torch.empty(d, dtype=torch.float32, device=Xd.device)
        Xc = torch.empty_like(Xd)
        L.check(L.lib().hlmc_km_center(L.stream(), Xd.data_ptr(), n, d, mean.data_ptr(), var.data_ptr(),
                                       Xc.data_ptr()), "hlmc_km_center")
        return mean, var, Xc

    def _sqdist(self, Xc, cand):
        n, d = Xc.shape
        out = torch.empty(len(cand), n, dtype=torch.float32, device=Xc.device)
        L.check(L.lib().hlmc_km_sqdist_rows(L.stream(), Xc.data_ptr(), n, d, L.i64_array(cand), len(cand),
                                            out.data_ptr()), "hlmc_km_sqdist_rows")
        return out

    def _draw_seeds(self, rs, n, n_init, mine):
        """Consume the one RandomState stream exactly as sklearn's sequential restarts do (data-independent
        counts, seeding_draws): per restart the first centre's choice(n, p=w / w.sum()) and the k - 1 per-centre
        uniform(size=trials) vectors -- kept for this rank's restarts, drawn and discarded for the others."""
        k = self.n_clusters
        trials = 2 + int(np.log(k))
        w = np.ones(n, dtype=np.float32)
        # rs.choice(n, p=w / w.sum()) is one random_sample() searched in the normalised float64 cdf of p
        # (numpy mtrand.RandomState.choice); the cdf is the same for every restart, so it is built once
        cdf = np.array(w / w.sum(), dtype=np.float64).cumsum()
        cdf /= cdf[-1]
        draws = {}
        for i in range(n_init):
            if i not in mine:
                rs.random_sample(self.seeding_draws(k))
                continue
            cid = int(cdf.searchsorted(rs.random_sample(), side="right"))
            draws[i] = (cid, [rs.uniform(size=trials) for _ in range(1, k)])
        return draws, trials

    def _kmeans_plusplus_batch(self, Xc, seeds, trials):
        """sklearn _kmeans_plusplus for R restarts in lockstep (one launch per stage for all of them): the
        candidate draw (searchsorted of the float64 cumsum, hlmc_km_pp_search) and the candidates' distances with
        the running minimum (hlmc_km_pp_dist) on the device; the host keeps sklearn's float32 BLAS potentials
        (closest @ w, dist @ w: numpy on the copied-back distances) and argmin, and redoes with numpy the rare
        draws the device's error bracket flags as undecidable."""
        n, d = Xc.shape
        k, R, T = self.n_clusters, len(seeds), trials
        dev = Xc.device
        lib = L.lib()
        w = np.ones(n, dtype=np.float32)
        idx = np.full((R, k), -1, dtype=np.int64)
        idx[:, 0] = [c for c, _ in seeds]
        cand = torch.as_tensor(idx[:, 0].copy(), device=dev)
        prev = torch.empty(R, 1, n, dtype=torch.float32, device=dev)
        L.check(lib.hlmc_km_pp_dist(L.stream(), Xc.data_ptr(), n, d, R, 1, cand.data_ptr(), None, 1, None,
                                    prev.data_ptr()), "hlmc_km_pp_dist")
        prev_h = prev.cpu().numpy()
        pots = [prev_h[r] @ w for r in range(R)]               # closest_dist_sq @ sample_weight: float32 (1,)
        best = np.zeros(R, dtype=np.int32)
        bufs = [torch.empty(R, T, n, dtype=torch.float32, device=dev) for _ in range(2)]
        cand = torch.empty(R * T, dtype=torch.int64, device=dev)
        amb = torch.empty(R * T, dtype=torch.int32, device=dev)
        # two pinned host images of the distances (this step's and the previous step's closest rows)
        pins = [_pinned_like(b) for b in bufs]
        cpin, apin = _pinned_like(cand), _pinned_like(amb)
        for c in range(1, k):
            out = bufs[c % 2]
            rv = np.stack([seeds[r][1][c - 1] * pots[r] for r in range(R)]).astype(np.float64)   # rand_vals
            prevT = prev.shape[1]
            bh = best.ctypes.data_as(C.POINTER(C.c_int32))
            L.check(lib.hlmc_km_pp_search(L.stream(), n, R, T, prev.data_ptr(), prevT, bh,
                                          np.ascontiguousarray(rv).ctypes.data_as(C.POINTER(C.c_double)),
                                          cand.data_ptr(), amb.data_ptr()), "hlmc_km_pp_search")
            L.check(lib.hlmc_km_pp_dist(L.stream(), Xc.data_ptr(), n, d, R, T, cand.data_ptr(), prev.data_ptr(),
                                        prevT, bh, out.data_ptr()), "hlmc_km_pp_dist")
            # one synchronisation per step: the distances, candidates and flags
            out_h, cand_h, amb_h = _copy_back(dev, [(pins[c % 2], out), (cpin, cand), (apin, amb)])
            cand_h, amb_h = cand_h.reshape(R, T).copy(), amb_h.reshape(R, T)
            for r in range(R):
                closest = prev_h[r, best[r]][None, :]
                dist = out_h[r]
                if amb_h[r].any():
                    # numpy's own cumsum / searchsorted for this restart's draw (the device bracket could not decide)
                    cc = np.searchsorted(np.cumsum(w * closest, axis=None, dtype=np.float64), rv[r])
                    np.clip(cc, None, closest.size - 1, out=cc)
                    cand_h[r] = cc
                    dist = self._sqdist(Xc, [int(x) for x in cc]).cpu().numpy()
                    np.minimum(closest, dist, out=dist)
                    out[r].copy_(torch.from_numpy(dist))
                    out_h[r] = dist
                cpot = dist @ w.reshape(-1, 1)
                b = int(np.argmin(cpot))
                pots[r] = cpot[b]
                best[r] = b
                idx[r, c] = cand_h[r, b]
            prev, prev_h = out, out_h
        cent = Xc[torch.as_tensor(idx.reshape(-1), device=dev)].reshape(R, k, d).contiguous()
        return cent, idx

    def _lloyd_batch(self, Xc, centers, tol):
        """sklearn _kmeans_single_lloyd for R restarts in lockstep: one assign / partitioned-sums / centre-update
        launch per iteration for all running restarts, one small copy back per iteration (label-change counts,
        centre shifts, the new centres) for sklearn's host-side tests: strict convergence (labels unchanged),
        sum(shift^2) <= tol, max_iter; a restart with an empty cluster is updated on the host that iteration
        (sklearn _relocate_empty_clusters_dense on host copies, as before)."""
        n, d = Xc.shape
        k, R = self.n_clusters, centers.shape[0]
        dev = Xc.device
        lib = L.lib()
        cbuf = [centers.contiguous(), torch.empty_like(centers)]
        labels = [torch.full((R, n), -1, dtype=torch.int32, device=dev), torch.empty(R, n, dtype=torch.int32, device=dev)]
        # [info R*(k+1) | changed R (int32 bits)]: one copy back per iteration together with the new centres
        pack = torch.empty(R * (k + 1) + R, dtype=torch.float32, device=dev)
        info = pack[:R * (k + 1)]
        changed = pack[R * (k + 1):].view(torch.int32)
        sums = torch.empty(R, k, d, dtype=torch.float32, device=dev)
        wts = torch.empty(R, k, dtype=torch.float32, device=dev)
        ws_bytes = int(lib.hlmc_km_sums_workspace(n, k)) * R
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        old_c = cbuf[0].cpu().numpy()
        pack_p, cen_p = _pinned_like(pack), _pinned_like(centers)
        final_c = old_c.copy()
        final_lab = torch.empty(R, n, dtype=torch.int32, device=dev)
        n_iter = np.zeros(R, dtype=np.int64)
        strict = np.zeros(R, dtype=bool)
        active = (1 << R) - 1
        Xh = None
        for it in range(self.max_iter):
            if not active:
                break
            cur, nxt = cbuf[it % 2], cbuf[(it + 1) % 2]
            lab_old, lab_new = labels[it % 2], labels[(it + 1) % 2]
            changed.zero_()
            L.check(lib.hlmc_km_assign_batch(L.stream(), Xc.data_ptr(), n, d, cur.data_ptr(), k, R, active,
                                             lab_new.data_ptr(), lab_old.data_ptr(), changed.data_ptr()))
            L.check(lib.hlmc_km_sums_batch(L.stream(), Xc.data_ptr(), n, d, lab_new.data_ptr(), k, R, active,
                                           sums.data_ptr(), wts.data_ptr(), ws.data_ptr(), ws_bytes))
            L.check(lib.hlmc_km_update_batch(L.stream(), k, d, R, active, sums.data_ptr(), wts.data_ptr(),
                                             cur.data_ptr(), nxt.data_ptr(), info.data_ptr()))
            # one synchronisation per iteration: counts, shifts and the new centres
            pack_h, nxt_h = _copy_back(dev, [(pack_p, pack), (cen_p, nxt)])
            info_h = pack_h[:R * (k + 1)].reshape(R, k + 1)
            chg = pack_h[R * (k + 1):].view(np.int32)
            for r in range(R):
                if not (active >> r) & 1:
                    continue
                if info_h[r, k] != 0:   # an empty cluster: this restart's update on the host, as sklearn does it
                    if Xh is None:
                        Xh = Xc.cpu().numpy()
                    new = sums[r].cpu().numpy()
                    wic = wts[r].cpu().numpy()
                    lab_h = lab_new[r].cpu().numpy()
                    dist = ((Xh - old_c[r][lab_h]) ** 2).sum(axis=1)
                    empty = np.where(wic == 0)[0]
                    if dist.max() > 0:
                        far = np.argpartition(dist, -empty.size)[:-empty.size - 1:-1]
                        for e, f in zip(empty, far):
                            o = lab_h[f]
                            new[o] -= Xh[f]
                            new[e] = Xh[f]
                            wic[e] = 1.0
                            wic[o] -= 1.0
                    amax = int(np.argmax(wic))
                    for j in range(k):
                        if wic[j] > 0:
                            new[j] *= np.float32(1.0 / float(wic[j]))
                        else:
                            new[j] = new[amax]
                    shift = np.sqrt(_euclid_f32(new, old_c[r])).astype(np.float32)
                    nxt[r].copy_(torch.from_numpy(new))
                else:
                    new = nxt_h[r].copy()
                    shift = np.sqrt(info_h[r, :k]).astype(np.float32)
                old_c[r] = new
                done = False
                if chg[r] == 0 and it > 0:
                    strict[r] = done = True
                elif (shift ** 2).sum() <= tol:
                    done = True
                elif it + 1 == self.max_iter:
                    done = True
                if done:
                    n_iter[r] = it + 1
                    final_c[r] = new
                    final_lab[r].copy_(lab_new[r])
                    active &= ~(1 << r)
        fc = torch.from_numpy(final_c).to(dev)
        redo = sum(1 << r for r in range(R) if not strict[r])
        if redo:   # not strictly converged: labels from the final centres (sklearn's last lloyd_iter, no update)
            L.check(lib.hlmc_km_assign_batch(L.stream(), Xc.data_ptr(), n, d, fc.data_ptr(), k, R, redo,
                                             final_lab.data_ptr(), None, None))
        inertia = torch.empty(R, dtype=torch.float32, device=dev)
        tmp = torch.empty(R, n, dtype=torch.float32, device=dev)
        L.check(lib.hlmc_km_inertia_batch(L.stream(), Xc.data_ptr(), n, d, fc.data_ptr(), k, final_lab.data_ptr(), R,
                                          inertia.data_ptr(), tmp.data_ptr()))
        return final_lab.cpu().numpy(), inertia.cpu().numpy().astype(np.float64), final_c, n_iter

    @staticmethod
    def seeding_draws(k):
        """Doubles one k-means++ seeding takes from the RandomState stream: choice(n, p) draws one, then each of
        the k - 1 further centres draws n_local_trials = 2 + int(ln k) (uniform(size=trials)); the count does
        not depend on the data."""
        return 1 + (k - 1) * (2 + int(np.log(k)))

    @staticmethod
    def _select_best(runs, k):
        """sklearn's best-of-n_init rule applied in restart order (sklearn/cluster/_kmeans.py, KMeans.fit):
        a later restart wins only with strictly lower inertia AND a different partition."""
        best = None
        for r in runs:
            if best is None or (r[2] < best[2] and not _is_same_clustering(r[1], best[1], k)):
                best = r
        return best

    def _device_x(self, X):
        """Rejecting NaN / infinity is sklearn's check_array.  Here it is also what keeps the kernels in bounds: a
        non-finite centre compares below no distance, the E-step then stores no cluster index and the kernels
        after it index the centres with the labels unchecked."""
        return L.device_matrix(X, self._dev(), finite=True)

    # ------------------------------------------------------------------ sklearn API
    def fit(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("sample_weight is not supported (the reference never passes it)")
        Xd = self._device_x(X)
        if Xd.shape[0] < self.n_clusters:
            raise ValueError(f"n_samples={Xd.shape[0]} should be >= n_clusters={self.n_clusters}")
        mean, var, Xc = self._center(Xd)
        return self._fit_centered(Xc, mean.cpu().numpy(), var.cpu().numpy())

    def _fit_centered(self, Xc, mean, var):
        """fit() on the centred device matrix and the host copies of hlmc_km_center's column mean and variance (all
        three the same for every k: kmeans_k_sweep computes them once).  The caller has checked n >= n_clusters."""
        n, d = Xc.shape
        tol = np.mean(var) * self.tol if self.tol else 0.0
        rs = self.random_state if isinstance(self.random_state, np.random.RandomState) \
            else np.random.RandomState(self.random_state)
        n_init = 1 if self.n_init == "auto" else int(self.n_init)
        world, rank = 1, 0
        if self.process_group is not None:
            world = dist.get_world_size(self.process_group)
            rank = dist.get_rank(self.process_group)
        mine = [i for i in range(n_init) if i % world == rank]
        seeds, trials = self._draw_seeds(rs, n, n_init, set(mine))
        runs = []
        # restarts in lockstep: <= 16 per batch, R x trials <= 64 (hlmc_km_pp_*), their candidate rows in LDS
        g = max(1, min(16, 64 // trials, (150 * 1024) // (8 * trials * (d + 1))))
        for g0 in range(0, len(mine), g):
            grp = mine[g0:g0 + g]
            c0, _ = self._kmeans_plusplus_batch(Xc, [seeds[i] for i in grp], trials)
            labels, inertia, centers, n_iter = self._lloyd_batch(Xc, c0, tol)
            for j, i in enumerate(grp):
                runs.append((i, labels[j], float(inertia[j]), centers[j], int(n_iter[j])))
        if world > 1:
            gathered = [None] * world
            dist.all_gather_object(gathered, runs, group=self.process_group)
            runs = sorted((r for part in gathered for r in part), key=lambda r: r[0])
        best = self._select_best(runs, self.n_clusters)
        self.labels_ = best[1].astype(np.int32)
        self.inertia_ = best[2]
        self.cluster_centers_ = best[3] + mean
        self.n_iter_ = best[4]
        self.n_features_in_ = d
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_

    def predict(self, X):
        Xd = self._device_x(X)
        dev = Xd.device
        n, d = Xd.shape
        if d != self.cluster_centers_.shape[1]:
            raise ValueError(f"X has {d} features, but KMeans was fitted with {self.cluster_centers_.shape[1]}")
        C_ = torch.as_tensor(self.cluster_centers_, device=dev).contiguous()
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        L.check(L.lib().hlmc_km_assign(L.stream(), Xd.data_ptr(), n, d, C_.data_ptr(), self.n_clusters,
                                       labels.data_ptr(), None, None))
        return labels.cpu().numpy()


def kmeans_k_sweep(X, k_range=range(2, 15), *, random_state=42, n_init=10, device=None):
    """The reference's K-Means search (src/Convolutional_VAE.py:311-329, src/Simple_VAE.py:244-251, the one sweep
    all three scripts share): X is uploaded, validated and centred once for all k, and all silhouettes come from one
    ``metrics.silhouette_scores`` call (one distance pass per label window instead of one per k).

    Returns ``(best_k, records)``.  ``records[i]`` describes ``k_range[i]``: ``k``, ``labels`` (int32, identical to
    ``KMeans(k, random_state=random_state, n_init=n_init).fit_predict(X)``), ``inertia`` and ``silhouette`` (the bits
    of ``metrics.silhouette_score(X, labels)``).  ``best_k`` follows the reference's rule: start at (2, -1) and
    replace on a strictly greater silhouette."""
    from . import metrics as M
    ks = [int(k) for k in k_range]
    first = KMeans(device=device)
    Xd = first._device_x(X)
    n = Xd.shape[0]
    if any(not 2 <= k <= n - 1 for k in ks):
        raise ValueError(f"every k must be in [2, n_samples - 1 = {n - 1}] (the silhouette is defined there only)")
    mean, var, Xc = first._center(Xd)
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    records = []
    for k in ks:
        km = KMeans(n_clusters=k, random_state=random_state, n_init=n_init, device=device)._fit_centered(Xc, mean, var)
        records.append({"k": k, "labels": km.labels_, "inertia": km.inertia_})
    sils = M.silhouette_scores(Xd, [r["labels"] for r in records]) if records else []
    best_k, best_sil = 2, -1
    for rec, sil in zip(records, sils):
        rec["silhouette"] = sil = float(sil)
        if sil > best_sil:
            best_sil, best_k = sil, rec["k"]
    return best_k, records


# ====================================================================================== DBSCAN
_DBSCAN_WORKSPACE_CAP = 24 << 30   # bytes of bit-packed adjacency held at once by a sweep (17 radii at n = 100,000)
_DBSCAN_MAX_RADII = 32             # radii per hlmc_dbscan_neighbors call


def _radius_sq(eps):
    """sklearn's float32 radius-neighbours path squares the radius in float32: the threshold the float64 squared
    distances are compared with is float64(float32(float32(eps) * float32(eps))), not eps ** 2."""
    e = np.float32(eps)
    return float(np.float32(e * e))


def _dbscan_chunks(Xd, eps_list, min_samples, workspace_cap=None):
    """One neighbourhood pass per chunk of radii (as many as the workspace cap holds, at most 32), then the
    labelling pass per radius.  Yields per chunk the list of its radii's (index, labels int64 [n], core mask bool [n],
    borderline pairs), in the order of eps_list; nothing is copied back before a chunk's last launch is queued."""
    if min_samples < 1:
        raise ValueError("min_samples must be >= 1")
    eps_list = [float(e) for e in eps_list]
    if not eps_list or any(not e > 0.0 for e in eps_list):
        raise ValueError("eps must be > 0")
    lib = L.lib()
    n, d = Xd.shape
    dev = Xd.device
    cap = _DBSCAN_WORKSPACE_CAP if workspace_cap is None else int(workspace_cap)
    if int(lib.hlmc_dbscan_workspace(n, 1)) <= 0:
        raise ValueError(f"DBSCAN: n_samples={n} is outside the supported range [1, 262144]")
    chunk = min(_DBSCAN_MAX_RADII, len(eps_list))   # the most radii whose adjacencies fit under the cap (>= 1)
    while chunk > 1 and int(lib.hlmc_dbscan_workspace(n, chunk)) > cap:
        chunk -= 1
    ws_bytes = int(lib.hlmc_dbscan_workspace(n, chunk))
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        for c0 in range(0, len(eps_list), chunk):
            grp = eps_list[c0:c0 + chunk]
            E = len(grp)
            r = (C.c_double * E)(*[_radius_sq(e) for e in grp])
            counts = torch.empty(E, n, dtype=torch.int32, device=dev)
            border = torch.empty(E, dtype=torch.int64, device=dev)
            labels = torch.empty(E, n, dtype=torch.int32, device=dev)
            core = torch.empty(E, n, dtype=torch.uint8, device=dev)
            # a chunk's workspace size was computed for `chunk` radii; a shorter last chunk fits in it
            L.check(lib.hlmc_dbscan_neighbors(L.stream(), Xd.data_ptr(), n, d, r, E, counts.data_ptr(),
                                              border.data_ptr(), ws.data_ptr(), ws_bytes), "hlmc_dbscan_neighbors")
            for e in range(E):
                L.check(lib.hlmc_dbscan_labels(L.stream(), n, E, e, int(min_samples), counts.data_ptr(), ws.data_ptr(),
                                               ws_bytes, labels[e].data_ptr(), core[e].data_ptr(), None),
                        "hlmc_dbscan_labels")
            lab_h = labels.cpu().numpy().astype(np.int64)
            core_h = core.cpu().numpy().astype(bool)
            border_h = border.cpu().numpy()
            yield [(c0 + e, lab_h[e], core_h[e], int(border_h[e])) for e in range(E)]


def _dbscan_pass(Xd, eps_list, min_samples, workspace_cap=None):
    """The radii of _dbscan_chunks one by one."""
    for grp in _dbscan_chunks(Xd, eps_list, min_samples, workspace_cap):
        yield from grp


class DBSCAN:
    """sklearn.cluster.DBSCAN for float32 data with the neighbourhoods and the labelling on the GPU
    (src/Convolutional_VAE.py:353-354,382: ``DBSCAN(eps=eps, min_samples=5).fit_predict(latent_matrix)``).

    ``labels_`` and ``core_sample_indices_`` are bit-identical to sklearn 1.7's brute-force float32 path:
    i and j are neighbours iff max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) <= float32(eps)^2 (squared in float32),
    evaluated in float64; clusters are numbered by their smallest core index; a border point joins the
    lowest-numbered cluster among its core neighbours.

    sklearn's ``algorithm='auto'`` switches to a KD-tree (direct differences, another rounding) when
    ``n_features <= 15``; this class always uses the brute-force arithmetic, so for d <= 15 the guarantee is
    against ``sklearn.cluster.DBSCAN(algorithm='brute')``.

    ``n_borderline_pairs_`` counts the pairs i < j whose squared distance lies within
    4 (d + 4) 2^-53 (|x_i|^2 + |x_j|^2) of the threshold: only those could be decided differently by another
    summation order of the dot product (sklearn's comes from a BLAS dgemm).  When it is 0 the labels equal
    sklearn's by construction.  It is reported, never acted on.
    """

    def __init__(self, eps=0.5, *, min_samples=5, metric="euclidean", device=None):
        if metric != "euclidean":
            raise ValueError("only metric='euclidean' (the reference's) is implemented")
        self.eps, self.min_samples, self.metric, self.device = eps, min_samples, metric, device

    def fit(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("sample_weight is not supported (the reference never passes it)")
        Xd = L.device_matrix(X, self.device)
        (_, labels, core, border), = _dbscan_pass(Xd, [self.eps], self.min_samples)
        self.labels_ = labels
        self.core_sample_indices_ = np.flatnonzero(core)
        idx = torch.as_tensor(self.core_sample_indices_, device=Xd.device)
        self.components_ = Xd[idx].cpu().numpy()
        self.n_features_in_ = Xd.shape[1]
        self.n_borderline_pairs_ = border
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_


def dbscan_eps_sweep(X, eps_range=np.arange(3.0, 20.0, 1.0), min_samples=5, *, device=None, workspace_cap=None):
    """The reference's DBSCAN radius search (src/Convolutional_VAE.py:347-374) with one neighbourhood pass for
    all radii (chunked to ``workspace_cap`` bytes of adjacency).

    Returns ``(best_eps, records)``.  ``records[i]`` describes ``eps_range[i]``: ``eps``, ``labels`` (int64,
    bit-identical to ``DBSCAN(eps, min_samples).fit_predict(X)``), ``n_clusters`` (noise excluded), ``n_noise``,
    ``n_borderline_pairs`` and ``silhouette`` (``metrics.silhouette_score(X, labels)`` with noise as a label of
    its own, as the reference passes it; ``None`` when the radius has fewer than 2 clusters).  ``best_eps`` is
    the first radius with the highest silhouette, or the reference's default 10.0 when no radius qualifies."""
    from . import metrics as M
    Xd = L.device_matrix(X, device)
    eps_list = [float(e) for e in np.asarray(eps_range, dtype=np.float64).reshape(-1)]
    records = []
    best_eps, best_sil = 5.0, -1
    for grp in _dbscan_chunks(Xd, eps_list, min_samples, workspace_cap):
        scored = []
        for i, labels, core, border in grp:
            n_clusters = int(labels.max()) + 1 if labels.size else 0
            n_noise = int((labels == -1).sum())
            records.append({"eps": eps_list[i], "labels": labels, "n_clusters": n_clusters, "n_noise": n_noise,
                            "n_borderline_pairs": border, "silhouette": None})
            if n_clusters >= 2:
                scored.append(records[-1])
        if scored:   # the chunk's qualifying radii in one distance pass, in radius order
            for rec, sil in zip(scored, M.silhouette_scores(Xd, [r["labels"] for r in scored])):
                rec["silhouette"] = sil = float(sil)
                if sil > best_sil:
                    best_sil, best_eps = sil, rec["eps"]
    if best_sil == -1:
        best_eps = 10.0
    return best_eps, records


# ====================================================================================== Ward agglomerative
_WARD_MAX_N = 32768


def _ward_device_x(X, device):
    Xd = L.device_matrix(X, device, finite=True)
    n = Xd.shape[0]
    if n < 2:
        raise ValueError(f"Found array with {n} sample(s) while a minimum of 2 is required by AgglomerativeClustering.")
    if n > _WARD_MAX_N:
        raise ValueError(f"AgglomerativeClustering: n_samples={n} is above the supported {_WARD_MAX_N} (the float64 "
                         f"distance matrix takes n^2 * 8 bytes)")
    return Xd


def _ward_tree(Xd):
    """The Ward tree of the float32 rows: (children int64 [n-1][2], distances float64 [n-1]), sklearn's ``children_``
    and ``distances_`` bit for bit.  Device: the float64 distance matrix and the nearest-neighbour chain (n - 1 raw
    merges).  Host, O(n log n) on the merge records: stable sort by height, union-find relabelling (row i creates
    cluster n + i, each row is (min, max))."""
    lib = L.lib()
    n, d = Xd.shape
    dev = Xd.device
    ws_bytes = int(lib.hlmc_ward_workspace(n))
    if ws_bytes <= 0:
        raise ValueError(f"AgglomerativeClustering: n_samples={n} is outside the supported range [2, {_WARD_MAX_N}]")
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)   # the distance matrix is its first n * n * 8 bytes
        ab = torch.empty(3, n - 1, dtype=torch.int32, device=dev)   # merge_a, merge_b, merge_size
        md = torch.empty(n - 1, dtype=torch.float64, device=dev)
        L.check(lib.hlmc_ward_pdist(L.stream(), Xd.data_ptr(), n, d, ws.data_ptr()), "hlmc_ward_pdist")
        L.check(lib.hlmc_ward_chain(L.stream(), n, ws.data_ptr(), ab[0].data_ptr(), ab[1].data_ptr(), md.data_ptr(),
                                    ab[2].data_ptr(), ws.data_ptr(), ws_bytes), "hlmc_ward_chain")
        ab_h = ab.cpu().numpy()
        md_h = md.cpu().numpy()
    return _ward_relabel(ab_h[0], ab_h[1], md_h, n)


def _ward_relabel(ma, mb, md, n):
    order = np.argsort(md, kind="mergesort")
    parent = list(range(2 * n - 1))
    children = np.empty((n - 1, 2), dtype=np.int64)
    ma, mb = ma.tolist(), mb.tolist()
    for row, m in enumerate(order.tolist()):
        pair = []
        for x in (ma[m], mb[m]):
            r = x
            while parent[r] != r:
                r = parent[r]
            while parent[x] != r:        # path compression
                parent[x], x = r, parent[x]
            pair.append(r)
        a, b = pair
        children[row, 0], children[row, 1] = (a, b) if a < b else (b, a)
        parent[a] = parent[b] = n + row
    return children, md[order]


def _ward_cut(children, n, n_clusters):
    """sklearn's _hc_cut: a max-heap of node ids (heapq on negated ids) from the root, n_clusters - 1 rounds of push
    then pushpop; label i goes to the leaves under heap[i] in heap-array order."""
    import heapq
    ch = children.tolist()
    nodes = [-(max(ch[-1]) + 1)]
    for _ in range(n_clusters - 1):
        a, b = ch[-nodes[0] - n]
        heapq.heappush(nodes, -a)
        heapq.heappushpop(nodes, -b)
    labels = np.zeros(n, dtype=np.int64)
    for i, node in enumerate(nodes):
        stack, leaves = [-node], []
        while stack:
            v = stack.pop()
            if v < n:
                leaves.append(v)
            else:
                stack.extend(ch[v - n])
        labels[leaves] = i
    return labels


class AgglomerativeClustering:
    """sklearn.cluster.AgglomerativeClustering with its defaults (Ward linkage, Euclidean metric, no connectivity)
    for float32 data, the tree built on the GPU (src/Convolutional_VAE.py:334-342,381:
    ``AgglomerativeClustering(n_clusters=k).fit_predict(latent_matrix)``).

    ``labels_``, ``children_`` and ``distances_`` are bit-identical to sklearn 1.7.2 (scipy 1.15
    ``hierarchy.ward``): float64 distances with scipy's pdist rounding, the nearest-neighbour chain with the
    Lance-Williams Ward update in one single-workgroup launch, then on the host a stable sort by height, the
    union-find relabelling and sklearn's heap cut.

    The float64 distance matrix takes n^2 * 8 bytes (sklearn needs the same), so 2 <= n_samples <= 32768 (8 GiB);
    the 100,000-row shape the K-Means and DBSCAN extras cover is out of scope here.  ``connectivity`` and
    ``distance_threshold`` are not implemented.
    """

    def __init__(self, n_clusters=2, *, metric="euclidean", linkage="ward", compute_distances=False, device=None,
                 connectivity=None, distance_threshold=None):
        if linkage != "ward":
            raise ValueError("only linkage='ward' (sklearn's default, the reference's) is implemented")
        if metric != "euclidean":
            raise ValueError("only metric='euclidean' (the only one Ward linkage accepts) is implemented")
        if connectivity is not None or distance_threshold is not None:
            raise ValueError("connectivity and distance_threshold are not implemented (the reference passes neither)")
        self.n_clusters, self.metric, self.linkage = n_clusters, metric, linkage
        self.compute_distances, self.device = compute_distances, device

    def fit(self, X, y=None):
        Xd = _ward_device_x(X, self.device)
        n, d = Xd.shape
        k = int(self.n_clusters)
        if not 1 <= k <= n:
            raise ValueError(f"n_clusters={self.n_clusters} must be in [1, n_samples={n}]")
        self.children_, distances = _ward_tree(Xd)
        if self.compute_distances:
            self.distances_ = distances
        self.n_clusters_ = k
        self.n_leaves_ = n
        self.n_connected_components_ = 1
        self.n_features_in_ = d
        self.labels_ = _ward_cut(self.children_, n, k)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


def agglomerative_k_sweep(X, k_range=range(2, 15), *, device=None):
    """The reference's agglomerative sweep (src/Convolutional_VAE.py:334-342): the reference refits the same Ward
    tree for every k; here one tree is built and cut once per k.

    Returns ``(best_k, records)``.  ``records[i]`` describes ``k_range[i]``: ``k``, ``labels`` (int64, identical to
    ``AgglomerativeClustering(k).fit_predict(X)``) and ``silhouette`` (``metrics.silhouette_score(X, labels)``).
    ``best_k`` follows the reference's rule: start at (2, -1) and replace on a strictly greater silhouette."""
    from . import metrics as M
    Xd = _ward_device_x(X, device)
    n = Xd.shape[0]
    ks = [int(k) for k in k_range]
    if any(not 2 <= k <= n - 1 for k in ks):
        raise ValueError(f"every k must be in [2, n_samples - 1 = {n - 1}] (the silhouette is defined there only)")
    children, _ = _ward_tree(Xd)
    records = [{"k": k, "labels": _ward_cut(children, n, k)} for k in ks]
    sils = M.silhouette_scores(Xd, [r["labels"] for r in records]) if records else []   # one distance pass for all cuts
    best_k, best_sil = 2, -1
    for rec, sil in zip(records, sils):
        rec["silhouette"] = sil = float(sil)
        if sil > best_sil:
            best_sil, best_k = sil, rec["k"]
    return best_k, records
