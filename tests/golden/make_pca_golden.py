"""Records sklearn 1.7.2's PCA(svd_solver="full") on the float32 inputs of tests/pca_check.py, one
tests/golden/pca_<case>.npz per case: the attributes (k components), the first rows of fit_transform, and rho, the
residual of numpy's eigh on the exact Gram matrix (pca_check.Exact).  Run from the repository root:
    python -m tests.golden.make_pca_golden
"""
import warnings

import numpy as np
import sklearn
from sklearn.decomposition import PCA

from tests import pca_check as K


def record(name):
    X = K.case_input(name)
    c = K.CASES.get(name, dict(k=3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # the all-constant input divides 0 by 0
        sk = PCA(n_components=c["k"], svd_solver="full", whiten=c.get("whiten", False))
        T = sk.fit_transform(X)
    rho = K.exact(name).rho if name in K.CASES else 0.0
    np.savez_compressed(
        K.fixture_path(name), n=X.shape[0], d=X.shape[1], sklearn_version=sklearn.__version__,
        components=sk.components_, explained_variance=sk.explained_variance_,
        explained_variance_ratio=sk.explained_variance_ratio_, singular_values=sk.singular_values_, mean=sk.mean_,
        noise_variance=np.float64(sk.noise_variance_), n_components=sk.n_components_,
        transform=T[:K.FIXTURE_ROWS], rho=rho)
    print(f"{name:12s} n{X.shape[0]} d{X.shape[1]} k{sk.n_components_} rho {rho:.3e}")


if __name__ == "__main__":
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    for name in K.CASE_NAMES + [K.CONSTANT]:
        record(name)
