"""Record sklearn 1.7.2 Ward results as fixtures under tests/golden/ (run from the repository root):

    python tests/golden/make_ward_golden.py

For every case of tests/ward_check.py (seeded Gaussians, offset blobs, an integer grid, duplicate rows and the stored
oracle latents) ``sklearn.cluster.AgglomerativeClustering(n_clusters=k, compute_distances=True)`` is fitted for
k = 2..14.  A fixture holds only n, d, ``children_`` (int32), ``distances_`` (float64) and the labels of every k
(int16 [13][n]); the inputs are regenerated from their seeds.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import AgglomerativeClustering

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import ward_check as K  # noqa: E402


def main():
    os.chdir(ROOT)
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    for name in K.CASE_NAMES:
        X = K.case_input(name)
        n, d = X.shape
        labels = []
        for k in K.K_RANGE:
            sk = AgglomerativeClustering(n_clusters=k, compute_distances=True).fit(X)
            labels.append(sk.labels_.astype(np.int16))
            if k == K.K_RANGE[0]:
                children, distances = sk.children_, sk.distances_
            else:       # the reference refits the same tree for every k
                assert np.array_equal(children, sk.children_) and distances.tobytes() == sk.distances_.tobytes()
        np.savez_compressed(K.fixture_path(name), n=np.int64(n), d=np.int64(d), children=children.astype(np.int32),
                            distances=distances.astype(np.float64), labels=np.stack(labels),
                            k=np.array(list(K.K_RANGE), dtype=np.int64))
        print(f"{name}: n={n} d={d} {os.path.getsize(K.fixture_path(name))} bytes")


if __name__ == "__main__":
    main()
