"""Records tests/golden/tsne_fits.npz from live sklearn (run from the repository root:
``python -m tests.golden.make_tsne_golden``).

For each whole-fit case of tests/tsne_check.py (FIT_CASES) and random_state 0..7, sklearn's
``TSNE(n_components=2, perplexity=..., random_state=s)`` with its default arguments is fitted and two figures are
kept: the EXACT float64 KL divergence of its final embedding, recomputed by the helper from sklearn's own P (not
sklearn's Barnes-Hut estimate ``kl_divergence_``, which is recorded next to it for orientation), and
``trustworthiness(X, Y, n_neighbors=5)``.  The ARI of ``KMeans(k, n_init=10, random_state=0)`` on the embedding
against the blobs is recorded as well.
"""
import numpy as np
import sklearn
from sklearn.cluster import KMeans
from sklearn.manifold import TSNE, trustworthiness
from sklearn.metrics import adjusted_rand_score

from tests import tsne_check as K

SEEDS = tuple(range(8))


def main():
    out = {"sklearn_version": np.array(sklearn.__version__), "seeds": np.array(SEEDS)}
    for name, c in K.FIT_CASES.items():
        X, y = K.fit_input(name)
        P = K.sklearn_joint(X, c["perplexity"])
        kl, kl_bh, trust, ari = [], [], [], []
        for s in SEEDS:
            m = TSNE(n_components=2, perplexity=c["perplexity"], random_state=s)
            Y = m.fit_transform(X)
            kl.append(K.exact_kl(P.indptr, P.indices, P.data.astype(np.float32), Y))
            kl_bh.append(float(m.kl_divergence_))
            trust.append(float(trustworthiness(X, Y, n_neighbors=5)))
            lab = KMeans(c["centres"], n_init=10, random_state=0).fit_predict(Y)
            ari.append(float(adjusted_rand_score(y, lab)))
            assert m.n_iter_ == 999
        out[f"{name}_kl_exact"] = np.array(kl)
        out[f"{name}_kl_barnes_hut"] = np.array(kl_bh)
        out[f"{name}_trustworthiness"] = np.array(trust)
        out[f"{name}_ari"] = np.array(ari)
        out[f"{name}_learning_rate"] = np.array(float(m.learning_rate_))
        print(name, "KL exact", min(kl), max(kl), "BH", min(kl_bh), max(kl_bh), "trust", min(trust), max(trust),
              "ARI", min(ari))
    np.savez(K.FIT_FIXTURE, **out)


if __name__ == "__main__":
    main()
