"""SHA-256 of every output of the clustering / decomposition ops built on the float64 tile and the workspace carver
(csrc/dbscan.hip, ward.hip, pca.hip, metrics.hip) on seeded inputs at the fixture shapes, of the k-means ops
(csrc/kmeans.hip) and one whole KMeans fit, and of the mel / chroma ops (csrc/features.hip) with their workspace sizes
(those queries need a plan, and a plan uploads tables); with `--ws-only`, every plan-free *_workspace query over a grid
of sizes instead (host functions: no GPU needed).  A refactor of those files must leave every line of both listings as
it was:
    python scripts/cluster_hashes.py [--ws-only] --compare <parent libhlmc.so> <new libhlmc.so> [out.txt]
runs the listing once per library (HLMC_LIB), each in a child process of its own, writes the first listing with one
`same` / `DIFFERENT` mark per line and exits non-zero on any difference.  Without --compare it prints the listing of
the library HLMC_LIB selects."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1336, 128, 32), (1336, 64, 32), (4096, 64, 32), (1336, 370, 32), (1336, 290, 64), (2500, 16, 8)]  # n, d, q
K = 10


def workspace_lines(lib):
    ns = (1, 2, 63, 64, 65, 1336, 4096, 32768, 100000, 262144, 0, -1, 32769, 262145, (1 << 24) + 1)
    ds = (1, 3, 64, 65, 128, 370, 1024, 0, 1025)
    ks = (2, 10, 14, 1024)
    for n in ns:
        yield f"ws ward n={n}: {lib.hlmc_ward_workspace(n)}"
        for E in (1, 17, 32, 0, 33):
            yield f"ws dbscan n={n} E={E}: {lib.hlmc_dbscan_workspace(n, E)}"
        for d in ds:
            yield f"ws pca n={n} d={d}: {lib.hlmc_pca_workspace(n, d)}"
        for k in ks:
            yield f"ws silhouette n={n} k={k}: {lib.hlmc_silhouette_workspace(n, k)}"
    for k in ks:
        for d in ds:
            yield f"ws cluster_scores k={k} d={d}: {lib.hlmc_cluster_scores_workspace(k, d)}"
    for n in (1, 1023, 1024, 1025, 4097, 100000):
        for k in (1, 2, 10, 8192):
            yield f"ws km_sums n={n} k={k}: {lib.hlmc_km_sums_workspace(n, k)}"
    for c in (1, 32, 64, 96, 512, 0):
        yield f"ws op_bn_bwd C={c}: {lib.hlmc_op_bn_bwd_workspace(c)}"
    for ci, co in ((32, 64), (64, 128), (64, 32), (128, 64), (128, 256), (256, 512), (512, 512), (512, 256), (256, 128)):
        yield f"ws op_halo Ci={ci} Co={co}: {lib.hlmc_op_halo_workspace(ci, co)}"
    for n, cols in ((1, 1), (63, 7), (64, 7), (129, 3), (16384, 513), (16385, 513), (100000, 16384)):
        yield f"ws colstats n={n} cols={cols}: {lib.hlmc_colstats_workspace(n, cols)}"


def output_lines(lib, L):
    import numpy as np
    import torch
    dev = torch.device("cuda")

    def digest(*ts):
        h = hashlib.sha256()
        for t in ts:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
        return h.hexdigest()

    def buf(nbytes):
        return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)

    for n, d, q in SHAPES:
        rng = np.random.default_rng(7919 * n + d)
        centres = rng.normal(0.0, 3.0, (K, d))
        lab_h = rng.integers(0, K, n).astype(np.int32)
        X = torch.from_numpy((centres[lab_h] + rng.normal(0.0, 1.0, (n, d))).astype(np.float32)).to(dev)
        lab = torch.from_numpy(lab_h).to(dev)
        tag = f"n={n} d={d}"

        E = 3
        r = (C.c_double * E)(1.5 * d, 2.0 * d, 40.0 * d)
        ws = buf(lib.hlmc_dbscan_workspace(n, E))
        counts = torch.zeros(E, n, dtype=torch.int32, device=dev)
        border = torch.zeros(E, dtype=torch.int64, device=dev)
        L.check(lib.hlmc_dbscan_neighbors(L.stream(), X.data_ptr(), n, d, r, E, counts.data_ptr(), border.data_ptr(),
                                          ws.data_ptr(), ws.numel()), "hlmc_dbscan_neighbors")
        yield f"dbscan_neighbors {tag}: counts+borderline {digest(counts, border)} (sum {int(counts.sum())})"

        D = torch.zeros(n, n, dtype=torch.float64, device=dev)
        L.check(lib.hlmc_ward_pdist(L.stream(), X.data_ptr(), n, d, D.data_ptr()), "hlmc_ward_pdist")
        yield f"ward_pdist {tag}: D {digest(D)}"
        del D

        ws = buf(lib.hlmc_pca_workspace(n, d))
        mean = torch.zeros(d, dtype=torch.float64, device=dev)
        G = torch.zeros(d, d, dtype=torch.float64, device=dev)
        L.check(lib.hlmc_pca_cov(L.stream(), X.data_ptr(), n, d, mean.data_ptr(), G.data_ptr(), ws.data_ptr(),
                                 ws.numel()), "hlmc_pca_cov")
        yield f"pca_cov {tag}: mean+G {digest(mean, G)}"

        B = torch.from_numpy(rng.normal(0.0, 1.0, (d, q))).to(dev)
        o_off = torch.from_numpy(rng.normal(0.0, 1.0, q)).to(dev)
        out = torch.zeros(n, q, dtype=torch.float32, device=dev)
        L.check(lib.hlmc_pca_project(L.stream(), X.data_ptr(), n, d, B.data_ptr(), q, mean.data_ptr(), o_off.data_ptr(),
                                     out.data_ptr()), "hlmc_pca_project")
        yield f"pca_project {tag} q={q}: out {digest(out)}"

        if d <= 128:   # the silhouette kernel holds a row in registers: d <= 128
            ws = buf(lib.hlmc_silhouette_workspace(n, K))
            samples = torch.zeros(n, dtype=torch.float64, device=dev)
            score = torch.zeros(1, dtype=torch.float64, device=dev)
            L.check(lib.hlmc_silhouette(L.stream(), X.data_ptr(), n, d, lab.data_ptr(), K, samples.data_ptr(),
                                        score.data_ptr(), ws.data_ptr(), ws.numel()), "hlmc_silhouette")
            yield f"silhouette {tag} k={K}: samples+score {digest(samples, score)} ({float(score):.17g})"

        ws = buf(lib.hlmc_cluster_scores_workspace(K, d))
        out2 = torch.zeros(2, dtype=torch.float64, device=dev)
        L.check(lib.hlmc_cluster_scores(L.stream(), X.data_ptr(), n, d, lab.data_ptr(), K, out2.data_ptr(), ws.data_ptr(),
                                        ws.numel()), "hlmc_cluster_scores")
        yield f"cluster_scores {tag} k={K}: out {digest(out2)} ({float(out2[0]):.17g} {float(out2[1]):.17g})"
    yield from kmeans_lines(lib, L, digest, buf)
    yield from feature_lines(lib, L, digest, buf)
    torch.cuda.synchronize()


def kmeans_lines(lib, L, digest, buf):
    """The k-means ops one by one (R = 3 restarts where batched) on two seeded problems -- n = 4097 takes the partition
    path of the sums, d = 65 and d = 3 the d % 4 tails -- then one whole fit at the n = 1336, d = 128 fixture."""
    import numpy as np
    import torch
    import hlmc_amd
    from tests.golden import fixtures as FX
    dev, s, R = torch.device("cuda"), L.stream(), 3

    def f32(*shape):
        return torch.zeros(*shape, dtype=torch.float32, device=dev)

    for n, d, k in ((4097, 65, 5), (700, 3, 70)):
        rng = np.random.default_rng(31 * n + d + k)
        tag = f"n={n} d={d} k={k}"
        X = torch.from_numpy(rng.normal(0.0, 2.0, (n, d)).astype(np.float32)).to(dev)
        mean, var, Xc = f32(d), f32(d), f32(n, d)
        L.check(lib.hlmc_km_center(s, X.data_ptr(), n, d, mean.data_ptr(), var.data_ptr(), Xc.data_ptr()), "km_center")
        yield f"km_center {tag}: mean+var+Xc {digest(mean, var, Xc)}"
        for ncand in (5, 16):
            cand = [int(c) for c in rng.integers(0, n, ncand)]
            out = f32(ncand, n)
            L.check(lib.hlmc_km_sqdist_rows(s, Xc.data_ptr(), n, d, L.i64_array(cand), ncand, out.data_ptr()),
                    "km_sqdist_rows")
            yield f"km_sqdist_rows {tag} ncand={ncand}: out {digest(out)}"
        T = 4
        cand = torch.from_numpy(rng.integers(0, n, R * T)).to(dev)
        first, second = f32(R, T, n), f32(R, T, n)
        L.check(lib.hlmc_km_pp_dist(s, Xc.data_ptr(), n, d, R, T, cand.data_ptr(), None, 1, None, first.data_ptr()),
                "km_pp_dist")
        yield f"km_pp_dist {tag} R={R} T={T} no prev: out {digest(first)}"
        cand = torch.from_numpy(rng.integers(0, n, R * T)).to(dev)
        best = (C.c_int32 * R)(1, 3, 0)
        L.check(lib.hlmc_km_pp_dist(s, Xc.data_ptr(), n, d, R, T, cand.data_ptr(), first.data_ptr(), T, best,
                                    second.data_ptr()), "km_pp_dist")
        yield f"km_pp_dist {tag} R={R} T={T} prev: out {digest(second)}"
        cen = Xc[torch.from_numpy(rng.integers(0, n, R * k)).to(dev)].reshape(R, k, d).contiguous()
        lab = torch.zeros(R, n, dtype=torch.int32, device=dev)
        old = torch.zeros(R, n, dtype=torch.int32, device=dev)
        changed = torch.zeros(R, dtype=torch.int32, device=dev)
        act = (1 << R) - 1
        L.check(lib.hlmc_km_assign_batch(s, Xc.data_ptr(), n, d, cen.data_ptr(), k, R, act, lab.data_ptr(),
                                         old.data_ptr(), changed.data_ptr()), "km_assign_batch")
        yield f"km_assign_batch {tag} R={R}: labels+changed {digest(lab, changed)}"
        sums, w = f32(R, k, d), f32(R, k)
        ws = buf(R * lib.hlmc_km_sums_workspace(n, k))
        L.check(lib.hlmc_km_sums_batch(s, Xc.data_ptr(), n, d, lab.data_ptr(), k, R, act, sums.data_ptr(), w.data_ptr(),
                                       ws.data_ptr(), ws.numel()), "km_sums_batch")
        yield f"km_sums_batch {tag} R={R}: sums+weights {digest(sums, w)}"
        new, info = f32(R, k, d), f32(R, k + 1)
        L.check(lib.hlmc_km_update_batch(s, k, d, R, act, sums.data_ptr(), w.data_ptr(), cen.data_ptr(), new.data_ptr(),
                                         info.data_ptr()), "km_update_batch")
        yield f"km_update_batch {tag} R={R}: centres+info {digest(new, info)}"
        inertia, tmp = f32(R), f32(R, n)
        L.check(lib.hlmc_km_inertia_batch(s, Xc.data_ptr(), n, d, cen.data_ptr(), k, lab.data_ptr(), R,
                                          inertia.data_ptr(), tmp.data_ptr()), "km_inertia_batch")
        yield f"km_inertia_batch {tag} R={R}: inertia+rowdist {digest(inertia, tmp)}"
    km = hlmc_amd.KMeans(10, random_state=42, n_init=10).fit(FX.blobs(1336, 128, 10, seed=1336 + 128 + 10))
    fit = digest(torch.from_numpy(km.labels_), torch.from_numpy(np.ascontiguousarray(km.cluster_centers_)),
                 torch.tensor([km.inertia_], dtype=torch.float64))
    yield f"KMeans(10, random_state=42, n_init=10).fit n=1336 d=128: labels+centres+inertia {fit} (n_iter {km.n_iter_})"


def feature_lines(lib, L, digest, buf):
    """The mel / chroma ops at B = 65, an even and an odd clip length (pair-load and single-load STFT) and the plans
    n_mels = 128 and 40; then their workspace sizes over a grid."""
    import numpy as np
    import torch
    from hlmc_amd import features as F
    dev, s, B, keep, n_mfcc = torch.device("cuda"), L.stream(), 65, 20, 20
    for n_mels in (128, 40):
        p = F._plan(22050, 2048, 512, n_mels)
        for n in (8192, 8191):
            tag = f"B={B} n={n} n_mels={n_mels}"
            x = (0.3 * torch.randn(B, n, generator=torch.Generator().manual_seed(n + n_mels))).to(dev)
            T = int(lib.hlmc_mel_frames(p, n))
            rng = np.random.default_rng(n + n_mels)
            mean = torch.from_numpy(rng.normal(-40.0, 5.0, n_mels * keep)).to(dev)
            scale = torch.from_numpy(rng.uniform(0.5, 9.0, n_mels * keep)).to(dev)
            ws = buf(lib.hlmc_mel_workspace(p, B, n))
            out = torch.zeros(B, n_mels, T, device=dev)
            L.check(lib.hlmc_melspectrogram(p, s, x.data_ptr(), B, n, out.data_ptr(), ws.data_ptr()), "melspectrogram")
            yield f"melspectrogram {tag}: out {digest(out)}"
            out = torch.zeros(B, n_mels, keep, device=dev)
            L.check(lib.hlmc_mel_db(p, s, x.data_ptr(), B, n, keep, 1e-10, 80.0, out.data_ptr(), ws.data_ptr()), "mel_db")
            yield f"mel_db {tag} keep={keep}: out {digest(out)}"
            for dtype, code in ((torch.float32, L.HLMC_F32), (torch.bfloat16, L.HLMC_BF16)):
                out = torch.zeros(B, n_mels, keep, dtype=dtype, device=dev)
                L.check(lib.hlmc_mel_db_zscore(p, s, x.data_ptr(), B, n, keep, 1e-10, 80.0, mean.data_ptr(),
                                               scale.data_ptr(), code, out.data_ptr(), ws.data_ptr()), "mel_db_zscore")
                yield f"mel_db_zscore {tag} keep={keep} {str(dtype)[6:]}: out {digest(out)}"
            out = torch.zeros(B, n_mfcc, T, device=dev)
            L.check(lib.hlmc_mfcc(p, s, x.data_ptr(), B, n, n_mfcc, out.data_ptr(), ws.data_ptr()), "mfcc")
            yield f"mfcc {tag} n_mfcc={n_mfcc}: out {digest(out)}"
            ws = buf(lib.hlmc_chroma_workspace(p, B, n))
            out, tun = torch.zeros(B, 12, T, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
            L.check(lib.hlmc_chroma_stft(p, s, x.data_ptr(), B, n, out.data_ptr(), tun.data_ptr(), ws.data_ptr()),
                    "chroma_stft")
            yield f"chroma_stft {tag}: out+tuning {digest(out, tun)}"
        for b in (1, 3, 64, 65, 256):
            for n in (8191, 8192, 65024):
                yield (f"ws mel B={b} n={n} n_mels={n_mels}: {lib.hlmc_mel_workspace(p, b, n)}  "
                       f"chroma: {lib.hlmc_chroma_workspace(p, b, n)}")


def listing(ws_only):
    sys.path.insert(0, ROOT)
    from hlmc_amd import _lib as L
    lib = L.lib()
    for line in workspace_lines(lib) if ws_only else output_lines(lib, L):
        print(line, flush=True)


def compare(lib_a, lib_b, ws_only, out):
    runs = []
    for path in (lib_a, lib_b):
        cmd = [sys.executable, os.path.abspath(__file__)] + (["--ws-only"] if ws_only else [])
        p = subprocess.run(cmd, env=dict(os.environ, HLMC_LIB=os.path.abspath(path)), capture_output=True, text=True,
                           timeout=600)
        if p.returncode != 0:
            print(f"{path}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            return 1
        runs.append(p.stdout.splitlines())
    a, b = runs
    bad = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    print(f"# {lib_a} vs {lib_b}: {len(a)} lines, {bad} different", file=out)
    for i, x in enumerate(a):
        print(f"{x}  [{'same' if i < len(b) and b[i] == x else 'DIFFERENT: ' + (b[i] if i < len(b) else 'missing')}]",
              file=out)
    return 1 if bad else 0


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--compare" in flags:
        out = open(args[2], "w") if len(args) > 2 else sys.stdout
        sys.exit(compare(args[0], args[1], "--ws-only" in flags, out))
    listing("--ws-only" in flags)
