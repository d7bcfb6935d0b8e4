"""SHA-256 of every output of the clustering / decomposition ops built on the float64 tile and the workspace carver
(csrc/dbscan.hip, ward.hip, pca.hip, metrics.hip) on seeded inputs at the fixture shapes; with `--ws-only`, every
*_workspace query over a grid of sizes instead (host functions: no GPU needed).  A refactor of those files must leave
every line of both listings as it was:
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
    torch.cuda.synchronize()


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
