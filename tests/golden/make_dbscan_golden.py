"""Record sklearn 1.7.2 DBSCAN results as fixtures under tests/golden/ (run from the repository root):

    python tests/golden/make_dbscan_golden.py

For every case of tests/dbscan_check.py (the stored oracle latents and the seeded uneven-density blobs) three radii are
read from the k-distance curve and ``sklearn.cluster.DBSCAN(eps, min_samples=5)`` is fitted (``algorithm='brute'`` for
d <= 15, where sklearn would otherwise switch to a KD-tree).  A fixture holds only the case parameters (eps,
min_samples, algorithm, n, d), the labels and the core sample indices; the inputs are regenerated from their seeds.
The generator fails when a case has no radius with >= 2 clusters, >= 1 noise point and >= 20 border points.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import DBSCAN

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import dbscan_check as K  # noqa: E402


def main():
    os.chdir(ROOT)
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    for name in K.CASE_NAMES:
        X = K.case_input(name)
        n, d = X.shape
        algorithm = "brute" if d <= 15 else "auto"
        radii = K.k_distance_radii(X, K.QUANTILES.get(name, K.DEFAULT_QUANTILES))
        out = dict(eps=np.array(radii, dtype=np.float64), min_samples=np.int64(K.MIN_SAMPLES),
                   algorithm=np.array(algorithm), n=np.int64(n), d=np.int64(d))
        rich = False
        for i, eps in enumerate(radii):
            sk = DBSCAN(eps=eps, min_samples=K.MIN_SAMPLES, algorithm=algorithm).fit(X)
            out[f"labels_{i}"] = sk.labels_.astype(np.int32)
            out[f"core_{i}"] = sk.core_sample_indices_.astype(np.int32)
            clusters, noise, border = K.stats(sk.labels_, sk.core_sample_indices_)
            rich |= clusters >= 2 and noise >= 1 and border >= 20
            print(f"{name}: eps={eps} clusters={clusters} noise={noise} border={border}")
        assert rich, f"{name}: no radius with >= 2 clusters, >= 1 noise point and >= 20 border points"
        np.savez_compressed(K.fixture_path(name), **out)


if __name__ == "__main__":
    main()
