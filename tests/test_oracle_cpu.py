"""CPU checks of the oracle itself against the reference's pins and the committed golden fixtures."""
import os

import numpy as np
import pytest
import torch

from oracle import kmeans_oracle as KO
from oracle import mel_oracle as MO
from oracle import models_oracle as OM
from tests import kmeans_cases as KC
from tests.golden import fixtures as FX

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_librosa_documented_filterbank_value():
    # librosa docs: filters.mel(sr=22050, n_fft=2048)[0, 1] ~= 0.016; 2018 non-zeros; band 0 = bins 1..4
    W = MO.mel_filterbank()
    assert abs(W[0, 1] - 0.016) < 5e-4
    assert (W > 0).sum() == 2018
    nz0 = np.nonzero(W[0])[0]
    nz127 = np.nonzero(W[127])[0]
    assert (nz0[0], nz0[-1]) == (1, 4) and (nz127[0], nz127[-1]) == (971, 1023)


def test_window_and_dct_match_scipy():
    """The two scipy primitives librosa's mel / MFCC path calls (src/1_preprocessing_advanced.py:99-106 via
    librosa.stft's get_window; src/1_preprocessing.py:61-70 via librosa.feature.mfcc's scipy.fftpack.dct), pinned
    against scipy itself (importable here and on the GPU box): the periodic Hann window bit for bit, the
    DCT-II ortho matrix to 1e-15."""
    import scipy.fftpack
    import scipy.signal
    for n in (2048, 1024, 400):
        np.testing.assert_array_equal(MO.hann_window(n), scipy.signal.get_window("hann", n, fftbins=True))
    D = scipy.fftpack.dct(np.eye(128), type=2, norm="ortho", axis=0)[:40]
    assert float(np.abs(MO.dct_ortho_matrix() - D).max()) <= 1e-15
    x = np.random.default_rng(3).standard_normal((128, 7))
    np.testing.assert_allclose(MO.dct_ortho_matrix() @ x, scipy.fftpack.dct(x, type=2, norm="ortho", axis=0)[:40],
                               rtol=0, atol=1e-13)


def test_frames_and_shapes():
    assert MO.n_frames(65024) == 128 and MO.n_frames(661500) == 1292
    y = MO.synthetic_pcm(1, 65024, seed=1)[0]
    assert MO.extract_mel_spectrogram(y).shape == (128, 128)
    assert MO.extract_mel_spectrogram(y, fixed_time_steps=1024).shape == (128, 1024)
    assert MO.mfcc(y).shape == (40, 128)


def test_mel_fixture_reproduces():
    fx = np.load("tests/golden/features.npz")
    y = MO.synthetic_pcm(2, 65024, seed=7)
    np.testing.assert_array_equal(np.stack([MO.extract_mel_spectrogram(c) for c in y]), fx["mel_db"])
    np.testing.assert_array_equal(MO.mel_filterbank(), fx["mel_basis"])


def test_db_properties():
    y = MO.synthetic_pcm(1, 65024, seed=3)[0]
    db = MO.extract_mel_spectrogram(y)
    assert db.max() == 0.0 and db.min() >= -80.0
    assert np.all(MO.extract_mel_spectrogram(np.zeros(65024, np.float32)) == 0.0)


@pytest.mark.parametrize("case", FX.KMEANS_CASES[:4], ids=lambda c: f"n{c[0]}_d{c[1]}_k{c[3]}")
def test_kmeans_oracle_matches_sklearn_fixture(case):
    n, d, centers, k, n_init = case
    X = FX.blobs(n, d, centers, seed=n + d + k)
    fx = np.load(f"tests/golden/kmeans_n{n}_d{d}_k{k}_i{n_init}.npz")
    km = KO.KMeans(k, random_state=42, n_init=n_init).fit(X)
    np.testing.assert_array_equal(km.labels_, fx["labels"])
    assert km.n_iter_ == int(fx["n_iter"])


@pytest.mark.parametrize("case", [c for c in FX.KMEANS_OVERLAP_CASES if c[0] * c[4] <= 14000],
                         ids=lambda c: f"n{c[0]}_d{c[1]}_s{c[3]}_k{c[4]}_i{c[5]}")
def test_kmeans_oracle_matches_sklearn_overlap_fixture(case):
    """Overlapping clusters: labels decided by float32 rounding at near-ties; the oracle's bit-level E-step
    restatement reproduces sklearn's labels, n_iter and inertia exactly."""
    n, d, true_k, spread, k, n_init = case
    X = FX.overlap_blobs(n, d, true_k, spread, FX.overlap_seed(case))
    fx = np.load("tests/golden/" + FX.overlap_fixture_name(case))
    km = KO.KMeans(k, random_state=42, n_init=n_init).fit(X)
    np.testing.assert_array_equal(km.labels_, fx["labels"])
    assert km.n_iter_ == int(fx["n_iter"]) and km.inertia_ == float(fx["inertia"])


@pytest.mark.parametrize("k", [2, 7, 14])
def test_kmeans_oracle_matches_sklearn_latent_fixture(k):
    fx = np.load("tests/golden/kmeans_latents_n1336_d128.npz")
    km = KO.KMeans(k, random_state=42, n_init=10).fit(fx["X"])
    np.testing.assert_array_equal(km.labels_, fx[f"labels_k{k}"])
    assert km.n_iter_ == int(fx[f"n_iter_k{k}"]) and km.inertia_ == float(fx[f"inertia_k{k}"])


@pytest.mark.parametrize("n,d,k", [(1336, 128, 2), (1336, 128, 10), (1000, 64, 5), (513, 100, 13), (257, 32, 16),
                                   (300, 130, 3), (77, 40, 1)])
def test_estep_restatement_matches_blas(n, d, k):
    """oracle estep_dist (the arithmetic hlmc_km_assign implements) == the sgemm call sklearn makes
    (scipy's OpenBLAS, column-major TN per 256-row chunk), bit for bit, on near-tie data."""
    from threadpoolctl import threadpool_info, threadpool_limits
    archs = {i.get("architecture") for i in threadpool_info() if i.get("internal_api") == "openblas"}
    if archs != {"SkylakeX"}:
        pytest.skip(f"the restatement is of the SkylakeX OpenBLAS kernels the fixtures were made with, not {archs}")
    rng = np.random.default_rng(n * 31 + d * 7 + k)
    C = rng.standard_normal((k, d)).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    if k >= 2:
        m, u = (C[0] + C[1]) / 2, C[1] - C[0]
        u = u / np.linalg.norm(u)
        X = (m + 0.3 * (X - np.outer(X @ u, u)) + np.outer(rng.standard_normal(n) * 1e-6, u)).astype(np.float32)
    cn = KO.row_norms_sq_f32(C)
    np.testing.assert_array_equal(cn, np.einsum("ij,ij->i", C, C))
    with threadpool_limits(1, "blas"):
        for s in range(0, n, KO.CHUNK):
            np.testing.assert_array_equal(KO.estep_dist(X[s:s + KO.CHUNK], C, cn),
                                          KO.estep_dist_blas(X[s:s + KO.CHUNK], C, cn))


@pytest.mark.parametrize("d", [3, 37, 130])
def test_sqdist_upcast_within_derived_bound_of_exact(d):
    """oracle sqdist_exact / sqdist_bound (the yardstick of the float64 distance kernels): sklearn's
    _euclidean_distances_upcast restatement stays inside the derived bound of the exact squared distance, on rows far
    from the origin with an exact duplicate, a one-ulp neighbour and a 1e-4 relative neighbour among the candidates."""
    X = KC.dup_rows(KC.SQDIST_N, d, seed=d)
    A = X[KC.SQDIST_CAND]
    exact = KO.sqdist_exact(A, X)
    bound = KO.sqdist_bound(A, X, d)
    assert exact.dtype == np.float64 and exact.shape == (len(KC.SQDIST_CAND), KC.SQDIST_N) and (exact >= 0).all()
    assert exact[0, 0] == 0.0 and exact[0, 1] == 0.0 and 0.0 < exact[0, 2] < exact[0, 3] < 1e-3 * exact[0, 5]
    # the exact value against an independent evaluation: the float64 sum of squared float64 differences is within
    # (d + 3) 2^-53 relative of it (no cancellation between its non-negative terms)
    direct = ((A.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    assert (np.abs(direct - exact) <= (d + 3) * 2.0 ** -53 * exact).all()
    err = np.abs(KO._sqdist_upcast(A, X).astype(np.float64) - exact)
    print(f"d={d}: worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("case", KC.FIT_CASES, ids=KC.FIT_IDS)
def test_kmeans_oracle_matches_live_sklearn_off_workload_shapes(case):
    """Every whole-fit input of tests/test_kmeans_ops_gpu.py (odd d, d < 32, k up to 55, n_init up to 20, an input
    whose empty clusters are relocated): the oracle's KMeans equals live single-thread sklearn -- labels, inertia and
    n_iter -- so the GPU tests may compare against the oracle alone."""
    import warnings
    from sklearn.cluster import KMeans as SK
    from threadpoolctl import threadpool_info, threadpool_limits
    archs = {i.get("architecture") for i in threadpool_info() if i.get("internal_api") == "openblas"}
    if archs != {"SkylakeX"}:     # as test_estep_restatement_matches_blas: live sklearn's labels follow the host's sgemm
        pytest.skip(f"the restatement is of the SkylakeX OpenBLAS kernels the fixtures were made with, not {archs}")
    name, kind, n, d, true_k, k, n_init = case
    X = KC.fit_input(case)
    assert X.shape == (n, d) and X.dtype == np.float32
    ours = KO.KMeans(k, random_state=42, n_init=n_init).fit(X)
    with threadpool_limits(1), warnings.catch_warnings():
        warnings.simplefilter("ignore")          # fewer distinct clusters than k on the repeated-row input
        ref = SK(n_clusters=k, random_state=42, n_init=n_init).fit(X)
    np.testing.assert_array_equal(ours.labels_, ref.labels_)
    assert ours.inertia_ == ref.inertia_ and ours.n_iter_ == ref.n_iter_


def test_scaler_oracle_matches_fixture():
    fx = np.load("tests/golden/features.npz")
    rng = np.random.default_rng(11)
    cols = (rng.standard_normal((64, 300)) * rng.uniform(0.1, 5, 300) + rng.uniform(-3, 3, 300)).astype(np.float32)
    cols[:, 5] = 2.5
    m, v, s = KO.standard_scaler_fit(cols)
    np.testing.assert_array_equal(s, fx["scaler_scale"])
    np.testing.assert_array_equal(KO.standard_scaler_transform(cols, m, s), fx["scaler_out"])


@pytest.mark.parametrize("name", ["audio_128x128", "hybrid_128x128_td768", "cvae_128x128", "simple_370"])
def test_model_oracle_reproduces_fixture(name):
    case = FX.case_by_name(name)
    fx = np.load(f"tests/golden/model_{name}.npz")
    torch.manual_seed(42)
    m = {"hybrid": OM.HybridVAE, "cvae": OM.ConditionalVAE, "simple": OM.VAE}[case["kind"]](**FX.oracle_ctor(case))
    assert [n for n, _ in m.named_parameters()] == list(fx["param_names"])
    np.testing.assert_array_equal(FX.param_summary(m), fx["param_checksum_init"])
    ins, eps = FX.inputs_fn(case)(0)
    torch.manual_seed(7)
    m.train()
    out = m(*ins, eps=eps)
    if case["kind"] == "simple":
        loss = OM.vae_loss(out[0], ins[0], out[1], out[2], beta=0.8)
    elif case["kind"] == "hybrid":
        loss = OM.loss_function(out[0], ins[0], out[1], ins[1], out[2], out[3])
    else:
        loss = OM.cvae_loss_function(out[0], ins[0], out[1], ins[1], out[2], out[3], beta=4.0)
    np.testing.assert_allclose([float(t) for t in loss], fx["loss_step0"], rtol=1e-6)
    loss[0].backward()
    np.testing.assert_allclose(FX.grad_summary(m), fx["grad_summary"], rtol=1e-5, atol=1e-7)


def test_native_shapes_match_reference_at_128x1024():
    torch.manual_seed(42)
    m = OM.HybridVAE()  # reference default (128 x 1024)
    assert m.audio_fc.weight.shape == (1024, 16384) and sum(p.numel() for p in m.parameters()) == 43272065


# ---------------------------------------------------------------- cluster-quality metrics (§8f rows 1, 4)
@pytest.mark.parametrize("case", FX.METRICS_CASES)
def test_metrics_oracle_matches_sklearn_fixtures(case):
    """The numpy restatement (the GPU tests' checker) reproduces sklearn's recorded scores; the host label
    metrics of hlmc_amd.metrics (ARI / NMI / purity) reproduce sklearn and the reference's calculate_purity."""
    from oracle import metrics_oracle as MO
    import hlmc_amd
    n, d, centers, k, n_init = case
    fx = np.load(os.path.join(GOLDEN, FX.metrics_fixture_name(case)))
    X = FX.blobs(n, d, centers, seed=n + d + k)
    y_true = FX.blob_labels(n, d, centers, seed=n + d + k)
    y_pred = np.load(os.path.join(GOLDEN, FX.kmeans_fixture_name(case)))["labels"].astype(np.int64)
    np.testing.assert_allclose(MO.silhouette_samples(X, y_pred), fx["silhouette_samples"], rtol=1e-5, atol=1e-6)
    assert abs(MO.silhouette_score(X, y_pred) - float(fx["silhouette"])) <= 1e-6 * abs(float(fx["silhouette"])) + 1e-7
    assert abs(MO.davies_bouldin_score(X, y_pred) - float(fx["davies_bouldin"])) <= 1e-6 * float(fx["davies_bouldin"])  # sklearn: float32 centroids
    assert abs(MO.calinski_harabasz_score(X, y_pred) - float(fx["calinski_harabasz"])) <= 1e-6 * float(fx["calinski_harabasz"])
    M = hlmc_amd.metrics
    assert abs(M.adjusted_rand_score(y_true, y_pred) - float(fx["ari"])) <= 1e-12
    assert abs(M.normalized_mutual_info_score(y_true, y_pred) - float(fx["nmi"])) <= 1e-12
    assert M.calculate_purity(y_true, y_pred) == float(fx["purity"])


def test_spectral_oracle_properties():
    """Pins the restatement of librosa's frame features (parity against librosa itself is unpinned):
    a bin-centred tone has its centroid and rolloff at the tone, zcr = 2 f / sr, rms = A / sqrt(2);
    silence gives zeros (the unnormalised branch of librosa.util.normalize)."""
    from oracle import spectral_oracle as SO
    sr, n = 22050, 22050 * 2
    f = 100 * sr / 2048.0                      # bin 100
    t = np.arange(n) / sr
    y = (0.5 * np.sin(2 * np.pi * f * t)).astype(np.float32)
    inner = slice(4, -4)
    c = SO.spectral_centroid(y)[0, inner]
    assert np.all(np.abs(c - f) < 2e-3)
    # Hann main lobe: |X| = (1/2, 1, 1/2) at bins 99..101 -> cumsum crosses 0.85 * 2 at bin 101
    assert np.all(SO.spectral_rolloff(y)[0, inner] == 101 * sr / 2048.0)
    bw = SO.spectral_bandwidth(y)[0, inner]
    # S_norm = (1/4, 1/2, 1/4) -> bandwidth = sqrt(1/2) df; the float32 quantisation floor of y spread over
    # 1025 bins adds a few percent (deviations up to 10 kHz weigh it)
    df = sr / 2048.0
    assert np.all((bw > np.sqrt(0.5) * df) & (bw < 1.06 * np.sqrt(0.5) * df))
    np.testing.assert_allclose(SO.zero_crossing_rate(y)[0, inner], 2 * f / sr, atol=1.5 / 2048)
    np.testing.assert_allclose(SO.rms(y)[0, inner], 0.5 / np.sqrt(2), rtol=2e-3)
    z = np.zeros(n, np.float32)
    assert not SO.spectral_stats(z).any()
    stats = SO.spectral_stats(y)
    assert stats.shape == (10,) and np.isfinite(stats).all()


def test_chroma_oracle_properties():
    """Pins the chroma_stft restatement (parity vs librosa unpinned): the filterbank is 12 x 1025 float32 with
    unit-L2 columns before the octave weighting (so every column's norm is that weight); an A tone lands on
    chroma 9 (base_c=True); the tuning estimate follows a detuned tone to within the 0.01-semitone histogram's
    piptrack error; silence gives tuning 0 and all-zero chroma."""
    from oracle import spectral_oracle as SO
    fb = SO.chroma_filterbank()
    assert fb.shape == (12, 1025) and fb.dtype == np.float32
    freqs = np.linspace(0, 22050, 2048, endpoint=False)[1:1025]
    octw = np.exp(-0.5 * (((np.log2(freqs / 27.5) - 5.0) / 2) ** 2))
    np.testing.assert_allclose(np.linalg.norm(fb[:, 1:].astype(np.float64), axis=0), octw, rtol=1e-5)
    t = np.arange(22050 * 3) / 22050
    for det in (0.0, 0.23, -0.31):
        f = 440 * 2 ** (det / 12)
        y = (0.3 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 1.5 * f * t)).astype(np.float32)
        ch, tun = SO.chroma_stft(y)
        assert abs(tun - det) <= 0.06, (det, tun)
        assert np.argmax(ch[:, 8:-8].mean(1)) == 9
    ch, tun = SO.chroma_stft(np.zeros(8192, np.float32))
    assert tun == 0.0 and not ch.any()


def test_philox_known_answers():
    """oracle/rng_oracle.py Philox4x32-10 against the Random123 known-answer vectors (kat_vectors: philox4x32_10)."""
    from oracle.rng_oracle import normals, philox4x32
    assert philox4x32((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert philox4x32((0xffffffff,) * 4, (0xffffffff,) * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert philox4x32((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == (
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    a = normals(4096, seed=1234)
    assert abs(float(a.mean())) < 0.05 and abs(float(a.std()) - 1) < 0.05
    np.testing.assert_array_equal(normals(8, seed=1234, offset=4096 - 8), a[-8:])


@pytest.mark.parametrize("name", ["audio_128x128", "hybrid_128x128_td768", "cvae_128x128", "simple_370"])
def test_oracle_training_chain_reproduces_fixture_latents(name):
    """The oracle's 3-step train chain (tests/test_models_gpu._oracle_trained: the fixture generator's Adam steps
    and dropout seeds) then eval-mode encode reproduces the reference classes' fixture eval_mu bit for bit on the
    generating host — the pin of the latent-extraction contract (src/Convolutional_VAE.py:286-303,
    src/Conditional_VAE.py:397-402, src/Simple_VAE.py:225-226) the GPU test compares the engine against."""
    from tests.test_models_gpu import _oracle_trained
    case = FX.case_by_name(name)
    ora = _oracle_trained(case)
    ins, _ = FX.inputs_fn(case)(0)
    with torch.no_grad():
        mu = ora.encode(*ins)[0]
    fx = np.load(f"tests/golden/model_{name}.npz")["eval_mu"]
    err = float(np.abs(mu.numpy() - fx).max())
    # bit-exact where the fixtures were generated (this container's CPU); Adam-amplified rounding elsewhere
    assert err == 0.0 or float(np.linalg.norm(mu.numpy() - fx) / np.linalg.norm(fx)) < 5e-2, err


def test_adam_restatement_matches_torch_float64():
    """oracle/optim_oracle.adam_step (the float64 yardstick of the GPU Adam tests) against torch.optim.Adam
    (foreach=False) on float64 CPU tensors: 5 steps with weight decay and a large eps, every element within 1e-14
    relative -- the parameters and exp_avg_sq relative to their own magnitude, exp_avg relative to |m| + |g + wd p|
    of the step (it is a difference of those two terms: where they cancel, two correct float64 evaluations in a
    different operation order, torch's lerp and the formula's, differ by more than 1e-14 of the small result)."""
    from oracle import optim_oracle as OO
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-3, weight_decay=1e-2)
    g = torch.Generator().manual_seed(5)
    ps = [torch.randn(s, dtype=torch.float64, generator=g).requires_grad_() for s in ((7, 13), (129,), (1,))]
    opt = torch.optim.Adam(ps, foreach=False, **hp)
    mine = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for p in ps]
    for step in range(1, 6):
        for i, p in enumerate(ps):
            p.grad = torch.randn(p.shape, dtype=torch.float64, generator=g) * 10.0 ** (i - 1)
        opt.step()
        scale_m = [np.abs(m) + np.abs(p.grad.numpy() + hp["weight_decay"] * q) for p, (q, m, v) in zip(ps, mine)]
        mine = [OO.adam_step(q, p.grad.numpy(), m, v, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], step)
                for p, (q, m, v) in zip(ps, mine)]
        for p, (q, m, v), sm in zip(ps, mine, scale_m):
            st = opt.state[p]
            assert int(st["step"]) == step
            for got, want, scale in ((q, p.detach(), None), (m, st["exp_avg"], sm), (v, st["exp_avg_sq"], None)):
                want = want.numpy()
                assert np.all(np.abs(got - want) <= 1e-14 * (np.abs(want) if scale is None else scale)), step


def test_loss_restatement_matches_torch_float64_autograd():
    """oracle/optim_oracle.loss_sums_and_grads against torch float64 autograd of the same three sums."""
    from oracle import optim_oracle as OO
    g = torch.Generator().manual_seed(6)
    ra, a = torch.randn(301, dtype=torch.float64, generator=g), torch.randn(301, dtype=torch.float64, generator=g)
    rt, t = torch.randn(17, dtype=torch.float64, generator=g), torch.randn(17, dtype=torch.float64, generator=g)
    mu = 3 * torch.randn(33, dtype=torch.float64, generator=g)
    lv = torch.rand(33, dtype=torch.float64, generator=g) * 18 - 12
    coef = (2.0, 700.0, 4.0)
    for x in (ra, rt, mu, lv):
        x.requires_grad_()
    s = (((ra - a) ** 2).sum(), ((rt - t) ** 2).sum(), (1 + lv - mu ** 2 - lv.exp()).sum())
    (0.5 * coef[0] * s[0] + 0.5 * coef[1] * s[1] - 0.5 * coef[2] * s[2]).backward()
    sums, dra, drt, dmu, dlv = OO.loss_sums_and_grads(*(x.detach().numpy() for x in (ra, a, rt, t, mu, lv)), coef)
    np.testing.assert_allclose(sums, [float(x.detach()) for x in s], rtol=1e-13)
    for got, x in ((dra, ra), (drt, rt), (dmu, mu), (dlv, lv)):
        np.testing.assert_allclose(got, x.grad.numpy(), rtol=1e-13, atol=1e-13 * float(x.grad.abs().max()))
    sums0, _, drt0, _, _ = OO.loss_sums_and_grads(ra.detach().numpy(), a.numpy(), None, None, mu.detach().numpy(),
                                                  lv.detach().numpy(), coef)
    assert sums0[1] == 0.0 and drt0 is None and sums0[0] == sums[0] and sums0[2] == sums[2]


# ---------------------------------------------------------------- metric / scaler op-level oracles and their bounds
def _sil_all_inputs():
    from tests import metrics_cases as MC
    return [(c[0], *MC.sil_input(c)[:2]) for c in MC.SIL_CASES] + [(k, *v) for k, v in MC.sil_semantic_inputs().items()]


def test_silhouette_float32_restatement_within_bounds_on_every_gpu_input():
    """The kernel's arithmetic restated in numpy float32 (sequential sum, no fma) stays inside sums_bound /
    samples_bound / score_bound on every input of tests/test_metrics_ops_gpu.py: a bound wrong as stated fails here,
    without a GPU."""
    from oracle import metrics_oracle as MT
    worst = [0.0, 0.0, 0.0]
    for name, X, y in _sil_all_inputs():
        d = X.shape[1]
        S, S32 = MT.silhouette_sums(X, y), MT.silhouette_sums_f32(X, y)
        s, s32 = MT.silhouette_from_sums(S, y), MT.silhouette_from_sums(S32, y)
        eS, es = np.abs(S32 - S), np.abs(s32 - s)
        assert (eS <= MT.sums_bound(S, d)).all(), name
        assert (es <= MT.samples_bound(s, d)).all(), name
        assert abs(s32.mean() - s.mean()) <= MT.score_bound(s, d), name
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[0] = max(worst[0], float(np.nanmax(eS / MT.sums_bound(S, d))))
        worst[1] = max(worst[1], float((es / MT.samples_bound(s, d)).max()))
        worst[2] = max(worst[2], abs(s32.mean() - s.mean()) / MT.score_bound(s, d))
    print("worst err / bound of the float32 restatement: S %.3f, samples %.3f, score %.3f" % tuple(worst))
    assert worst[0] > 0.01, "sums_bound is too slack to catch anything"


def test_silhouette_oracle_semantics_match_live_sklearn():
    from sklearn.metrics import silhouette_samples as sk_samples
    from oracle import metrics_oracle as MT
    from tests import metrics_cases as MC
    for name, (X, y) in MC.sil_semantic_inputs().items():
        ref = sk_samples(X, y)
        got = MT.silhouette_samples(X, y)
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6, err_msg=name)
    X, y = MC.sil_semantic_inputs()["singleton"]
    assert MT.silhouette_samples(X, y)[17] == 0.0
    X, y = MC.sil_semantic_inputs()["duplicates"]
    assert (MT.silhouette_samples(X, y)[y == 0] == 1.0).all()
    X, y = MC.sil_semantic_inputs()["identical_rows_in_two_clusters"]
    assert (MT.silhouette_samples(X, y)[y < 2] == 0.0).all()


def test_cluster_stats_oracle_bounds_contain_a_float64_evaluation_and_match_sklearn():
    """oracle cluster_stats (longdouble) against the plain float64 numpy evaluation within its own derived bounds on
    every input of the GPU test, and its sklearn branches against live sklearn on the degenerate sets."""
    from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score
    from oracle import metrics_oracle as MT
    from tests import metrics_cases as MC
    worst = [0.0, 0.0]
    for case in MC.CLU_CASES:
        X, y, k = MC.clu_input(case)
        st = MT.cluster_stats(X, y)
        assert (st["counts"] == np.bincount(y, minlength=k)).all() and (st["counts"] > 0).all(), case[0]
        X64 = X.astype(np.float64)
        cent = np.stack([X64[y == c].mean(0) for c in range(k)])
        assert (np.abs(cent - st["cent"]) <= st["cent_bound"]).all(), case[0]
        intra = np.array([np.sqrt(((X64[y == c] - cent[c]) ** 2).sum(1)).mean() for c in range(k)])
        assert (np.abs(intra - st["intra"]) <= st["intra_bound"]).all(), case[0]
        db, ch = MT.davies_bouldin_score(X, y), MT.calinski_harabasz_score(X, y)
        assert abs(db - st["db"]) <= st["db_bound"], (case[0], db, st["db"], st["db_bound"])
        assert abs(ch - st["ch"]) <= st["ch_bound"], (case[0], ch, st["ch"], st["ch_bound"])
        assert st["db_bound"] <= 1e-9 * st["db"] and st["ch_bound"] <= 1e-9 * st["ch"], case[0]
        worst = [max(worst[0], abs(db - st["db"]) / st["db_bound"]), max(worst[1], abs(ch - st["ch"]) / st["ch_bound"])]
    print("worst err / bound of numpy float64: DB %.4f, CH %.4f" % tuple(worst))
    for name, (X, y, db, ch) in MC.DEGENERATE.items():
        X = np.asarray(X, dtype=np.float32)
        st = MT.cluster_stats(X, y)
        assert st["db"] == pytest.approx(db, abs=1e-15) and st["ch"] == pytest.approx(ch, abs=1e-15), name
        assert davies_bouldin_score(X, y) == pytest.approx(db, abs=1e-7), name
        assert calinski_harabasz_score(X, y) == pytest.approx(ch, abs=1e-7), name


def test_scaler_oracle_matches_live_sklearn_and_its_bounds_contain_float64_numpy():
    from sklearn.preprocessing import StandardScaler as SK
    from oracle import scaler_oracle as SO
    from tests import scaler_cases as SC
    for n, cols in SC.COLSTATS_CASES:
        X = SC.colstats_input(n, cols)
        sk = SK().fit(X)
        mean, var, scale = SO.scaler_fit(X)
        np.testing.assert_allclose(mean, sk.mean_, rtol=1e-14, err_msg=str((n, cols)))
        np.testing.assert_allclose(var, sk.var_, rtol=1e-10, err_msg=str((n, cols)))
        np.testing.assert_allclose(scale, sk.scale_, rtol=1e-10, err_msg=str((n, cols)))
        if cols > SC.SHIFTED_COL:
            assert scale[SC.CONST_COL] == 1.0 and (n == 1 or abs(scale[SC.SHIFTED_COL] - 1e-2) < 5e-3)
        np.testing.assert_array_equal(SO.zscore(X, sk.mean_, sk.scale_), sk.transform(X))
        # numpy's float64 sums (pairwise, another order than the kernel's chunks) are inside the exact-sum bounds
        X64 = X.astype(np.float64)
        s, sb = SO.col_sums(X)
        assert (np.abs(X64.sum(0) - s) <= sb).all()
        m = s / n
        corr, cb, m2, mb = SO.col_centered(X, m)
        t = X64 - m
        assert (np.abs(t.sum(0) - corr) <= cb).all() and (np.abs((t * t).sum(0) - m2) <= mb).all()


def test_pool_and_db_restatements_within_bounds_on_every_gpu_input():
    from oracle import scaler_oracle as SO
    from tests import scaler_cases as SC
    for kind in SC.POOL_KINDS:
        for rows in SC.POOL_ROWS:
            for cols in SC.POOL_COLS:
                x = SC.pool_input(rows, cols, kind)
                m, mb, sd, sb = SO.row_mean_std(x)
                gm, gs = SO.row_mean_std_f64(x)
                assert (np.abs(gm - m) <= mb).all() and (np.abs(gs - sd) <= sb).all(), (kind, rows, cols)
                np.testing.assert_allclose(np.concatenate([gm, gs]), MO.mean_std_pool(x), rtol=1e-5, atol=1e-5)
    worst = 0.0
    for name, B, F, T, zero_clip, ref_max, top_db in SC.DB_CASES:
        S = SC.db_input(B, F, T, seed=B + F + T, zero_clip=zero_clip).reshape(B, -1)
        ref, bound, clamped = SO.power_to_db(S, ref_max=ref_max, top_db=top_db)
        got = SO.power_to_db_f32(S, ref_max=ref_max, top_db=top_db)
        err = np.abs(got - ref)
        assert (err <= bound).all(), (name, float((err / bound).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        if top_db is not None:
            assert clamped.any(), name
            for b in range(B):
                assert (got[b][clamped[b]] == got[b].max() - np.float32(top_db)).all(), name
        lib = np.stack([MO.power_to_db(s, ref=np.max if ref_max else 1.0, top_db=top_db) for s in S])
        np.testing.assert_allclose(got, lib, atol=1e-4)
    print("worst err / bound of the float32 dB restatement: %.3f" % worst)
