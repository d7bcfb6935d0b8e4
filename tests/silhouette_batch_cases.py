"""Inputs shared by the batched-silhouette tests (tests/test_silhouette_batch_gpu.py, tests/test_silhouette_batch_cpu.py),
built from tests/metrics_cases.py's ``normals`` and ``labels``: every label of every labelling occurs, as
hlmc_silhouette_batch's precondition demands (include/hlmc.h).  Shapes are the smallest at which the batched kernel can
go wrong: one labelling (the single path's shape edges), the reference's k sweep (more columns than one window, a
labelling that straddles a window boundary), a labelling wider than a window behind a small one, more labellings in
one window than the sweep has, the cap of 64 labellings, repeated labellings, n = 3, data far from the origin."""
import os
import re

import numpy as np

from tests import metrics_cases as MC

MAX_BATCH = 64      # labellings per hlmc_silhouette_batch call (include/hlmc.h)


def _documented_windows():
    """(columns per window, columns above the feature threshold, the threshold), read from include/hlmc.h's description
    of hlmc_silhouette_batch: "windows of 64 columns (58 for d > 64: ...".  csrc/metrics.hip pins the same values with a
    static_assert on sil_batch_kw_max, so header, library and these cases cannot drift apart unnoticed."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hlmc.h")).read()
    m = re.search(r"windows of (\d+) columns \((\d+) for[\s*]+d > (\d+)", src)
    assert m, "include/hlmc.h no longer states the batched silhouette's window widths"
    return tuple(int(g) for g in m.groups())


def kw_max(d):
    """Accumulator columns per window of the batched distance kernel at d features, as include/hlmc.h documents them."""
    wide, narrow, threshold = _documented_windows()
    return narrow if d > threshold else wide


SWEEP_KS = tuple(range(2, 15))          # the reference's k range: K = 104, offsets 0, 2, 5, ..., 90

# (id, n, d, ks, offset)
CASES = (
    [(f"one_d{d}", 203, d, (5,), 0.0) for d in (1, 32, 33, 64, 65, 128)]
    + [(f"one_n{n}", n, 12, (2,), 0.0) for n in (3, 63, 64, 65, 129)]
    + [(f"sweep_d{d}", 203, d, SWEEP_KS, 0.0) for d in (16, 128)]
    + [("wide_behind_small", 300, 16, (3, 129), 0.0),
       ("m40_k2", 130, 33, (2,) * 40, 0.0),
       ("m64_k2", 130, 33, (2,) * MAX_BATCH, 0.0),
       ("same_three_times", 203, 12, (5, 5, 5), 0.0),
       ("n3_two_labellings", 3, 12, (2, 2), 0.0),
       ("offset1000_d65", 300, 65, (4, 9), 1000.0)]
)
IDS = [c[0] for c in CASES]


def offsets(ks):
    return np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)


def straddlers(ks, kw):
    """Labellings whose columns [off, off + k) cross a multiple of kw."""
    off = offsets(ks)
    return [m for m, k in enumerate(ks) if off[m] // kw != (off[m] + k - 1) // kw]


def case_input(case):
    """(X float32 [n][d], labels int32 [M][n], ks)."""
    name, n, d, ks, off = case
    X = MC.normals(n, d, seed=1000 * n + 10 * d + len(ks), offset=off)
    if name == "n3_two_labellings":
        return X, np.array([[0, 0, 1], [0, 1, 1]], dtype=np.int32), ks
    if n == 3:
        return X, np.array([[0, 0, 1]], dtype=np.int32), ks
    if name == "same_three_times":
        y = MC.labels(n, ks[0], seed=n + d)
        return X, np.stack([y, y, y]), ks
    return X, np.stack([MC.labels(n, k, seed=n + d + k + 31 * m) for m, k in enumerate(ks)]), ks


def blobs(n, d, centres, seed, spread=6.0):
    """n rows around `centres` well-separated centres (float32)."""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, spread, (centres, d))
    return (c[rng.integers(0, centres, n)] + rng.normal(0.0, 1.0, (n, d))).astype(np.float32)
