"""The persistent item walk of the STFT kernel body (csrc/features.hip stft_mel_body, modes 0 / 1 / 2).

Items are (clip, 16-frame group) pairs; block j of XCD k starts at item k n / 8 + j and steps by gridDim / 8.  At the
batch sizes the API tests use, the default grid has one block per item, so the loop's second iteration, the next-item
prefetch (`have`), the re-fetch of a wave that had no frame in the previous item and the walk across a clip boundary
never run.  The test hook hlmc_test_stft_grid launches a given number of blocks instead: with B = 5 clips of T = 50
frames (4 groups of 16, 16, 16, 2 frames: 20 items) a grid of 8 gives every block 2 to 3 items (the 2-frame group is
followed by the next clip's 16-frame group, so waves 2 and 3 re-fetch) and a grid of 16 mixes 1- and 2-item blocks.

Per-frame arithmetic does not depend on the walk, and the per-clip max / min are atomics over exact values, so every
grid must give BIT-IDENTICAL outputs; the default grid is also held to the oracle at the tolerances of
test_features_gpu.py and test_spectral_gpu.py (restated next to each check).

The second half pins the isolation of frames: a non-finite sample may only reach the frames that contain it.  Every
wave writes the power bins of its frame to its own LDS row and the mel bands read whole 8-bin steps of it, up to 7
floats past bin 1024 for the plans whose top band ends there; those floats must be zeros of this block, not a
neighbour wave's bins (0 * NaN = NaN)."""
import contextlib
import functools

import numpy as np
import pytest

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import mel_oracle as MO
from oracle import spectral_oracle as SO

pytestmark = pytest.mark.gpu
DF = 22050 / 2048.0   # bin spacing (Hz): a rolloff that picks the neighbouring bin differs by exactly this


@contextlib.contextmanager
def stft_grid(blocks):
    """Launch the STFT kernels with `blocks` blocks (None: the default grid); always restores the default."""
    try:
        if blocks:
            L.check(L.lib().hlmc_test_stft_grid(blocks), "hlmc_test_stft_grid")
        yield
    finally:
        L.check(L.lib().hlmc_test_stft_grid(0), "hlmc_test_stft_grid")


def test_hook_rejects_bad_grids(cuda):
    try:
        for bad in (-8, 1, 7, 12, 20):
            assert L.lib().hlmc_test_stft_grid(bad) != 0, bad
        for ok in (8, 16, 256, 0):
            assert L.lib().hlmc_test_stft_grid(ok) == 0, ok
    finally:
        L.check(L.lib().hlmc_test_stft_grid(0), "hlmc_test_stft_grid")


# ------------------------------------------------------------------------------------------- 1. walk invariance
@functools.lru_cache(maxsize=None)
def _pcm(B, n):
    return MO.synthetic_pcm(B, n, seed=n % 97)   # shared by the cases of one length; no test writes to it


@functools.lru_cache(maxsize=None)
def _mel_ref(B, n):
    return MO.melspectrogram(_pcm(B, n))


def _as_tuple(out):
    if isinstance(out, dict):
        return tuple(out[k] for k in hlmc_amd.SPECTRAL_FEATURES)
    return out if isinstance(out, tuple) else (out,)


def _check_mel_db(got, y, keep):
    # test_features_gpu.py: float32 STFT vs the oracle's float64 one: 0.05 dB overall, 2e-3 dB above -60 dB
    ref = np.stack([MO.extract_mel_spectrogram(c, fixed_time_steps=keep) for c in y])
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, atol=0.05)
    assert np.abs(got - ref)[ref > -60].max() < 2e-3


def _check_spectral(got, y):
    # test_spectral_gpu.py: centroid / bandwidth 1e-5 + 0.05 Hz; rolloff <= 1% of frames one bin off; zcr exact; rms 1e-5
    for b in range(y.shape[0]):
        np.testing.assert_allclose(got["spectral_centroid"][b, 0], SO.spectral_centroid(y[b])[0], rtol=1e-5, atol=0.05)
        np.testing.assert_allclose(got["spectral_bandwidth"][b, 0], SO.spectral_bandwidth(y[b])[0], rtol=1e-5,
                                   atol=0.05)
        d = np.abs(got["spectral_rolloff"][b, 0] - SO.spectral_rolloff(y[b])[0])
        assert np.all((d == 0) | (np.abs(d - DF) < 1e-9)), d.max()
        assert (d > 0).mean() <= 0.01
        np.testing.assert_array_equal(got["zcr"][b, 0], SO.zero_crossing_rate(y[b])[0])
        np.testing.assert_allclose(got["rms"][b, 0], SO.rms(y[b])[0], rtol=1e-5, atol=1e-9)


def _check_chroma(got, y):
    c, tun = got
    for b in range(y.shape[0]):
        ref, rt = SO.chroma_stft(y[b])
        assert tun[b] == rt, (b, tun[b], rt)
        np.testing.assert_allclose(c[b], ref, rtol=1e-4, atol=1e-6)


def _check_power(got, B, n):
    ref = _mel_ref(B, n)
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-6 * ref.max())


def _check_mfcc(got, y):
    np.testing.assert_allclose(got, np.stack([MO.mfcc(c) for c in y]), atol=0.05, rtol=1e-3)


# name -> (the call, its oracle check)
OPS = {
    "melspectrogram": (lambda y: hlmc_amd.melspectrogram(y), lambda g, y: _check_power(g, *y.shape)),
    "mel_db": (lambda y: hlmc_amd.extract_mel_spectrogram(y), lambda g, y: _check_mel_db(g, y, None)),
    "mel_db_crop48": (lambda y: hlmc_amd.extract_mel_spectrogram(y, fixed_time_steps=48),
                      lambda g, y: _check_mel_db(g, y, 48)),
    "mel_db_pad52": (lambda y: hlmc_amd.extract_mel_spectrogram(y, fixed_time_steps=52),
                     lambda g, y: _check_mel_db(g, y, 52)),
    "mfcc40": (lambda y: hlmc_amd.mfcc(y, n_mfcc=40), _check_mfcc),
    "spectral": (lambda y: hlmc_amd.extract_spectral_features(y), _check_spectral),
    "chroma": (lambda y: hlmc_amd.chroma_stft(y, return_tuning=True), _check_chroma),
}


def _assert_walk_invariant(op, y, grids):
    call, check = OPS[op]
    with stft_grid(None):
        base = call(y)
    for g in grids:
        with stft_grid(g):
            other = call(y)
        for i, (a, b) in enumerate(zip(_as_tuple(base), _as_tuple(other))):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert np.array_equal(a, b), (op, g, i, int((a != b).sum()))
    check(base, y)


# B = 5, T = 1 + n // 512 = 50 for both lengths: 20 items; the default grid is 24 blocks (per = 3: one item per block),
# 8 blocks walk 2 to 3 items each, 16 blocks 1 or 2.  Even n: 8-byte sample-pair loads; odd n: 4-byte loads.
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("n", [25088, 25105])
def test_walk_is_bit_invariant_and_meets_oracle(cuda, n, op):
    assert MO.n_frames(n) == 50
    _assert_walk_invariant(op, _pcm(5, n), (8, 16))


@pytest.mark.parametrize("op", list(OPS))
def test_single_item_leaves_seven_xcd_ranges_empty(cuda, op):
    """B = 1, n = 1500: T = 3 frames, one item; under a grid of 8 the ranges of XCDs 0..6 are empty (their blocks
    only issue the unconditional first fetch) and waves 3 of the one working block have no frame."""
    _assert_walk_invariant(op, _pcm(1, 1500), (8,))


def test_odd_hop_spectral_and_chroma(cuda):
    """hop 441: frame 1 starts at sample -583, so one of its sample pairs is (x[-1], x[0]) and straddles the clip's
    start (an even hop never does; the mel path at this hop is in test_mel_plans_gpu.py).  Both halves of such a
    pair are separate range-checked loads: x[0] must survive.  Tolerances as in test_spectral_gpu.py."""
    hop = 441
    y = _pcm(2, 22050)
    c = hlmc_amd.spectral_centroid(y, hop_length=hop)
    bw = hlmc_amd.spectral_bandwidth(y, hop_length=hop)
    ch, tun = hlmc_amd.chroma_stft(y, hop_length=hop, return_tuning=True)
    assert c.shape == (2, 1, 51) and ch.shape == (2, 12, 51)
    for b in range(2):
        np.testing.assert_allclose(c[b, 0], SO.spectral_centroid(y[b], 22050, 2048, hop)[0], rtol=1e-5, atol=0.05)
        np.testing.assert_allclose(bw[b, 0], SO.spectral_bandwidth(y[b], 22050, 2048, hop)[0], rtol=1e-5, atol=0.05)
        ref, rt = SO.chroma_stft(y[b], 22050, 2048, hop)
        assert tun[b] == rt
        np.testing.assert_allclose(ch[b], ref, rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------- 2. non-finite isolation
HOP_ISO = 2048                 # = n_fft: frame t covers samples [2048 t - 1024, 2048 t + 1024), no overlap
N_ISO = 2048 * 12              # T = 13 frames, one item per clip; wave w takes frames w, w + 4, w + 8, w + 12
BAD_FRAMES = [1, 5, 9]         # the frames of wave 1; sample 2048 t is the centre of frame t (Hann weight 1)
MEL_PLANS = [(22050, 128), (16000, 80), (44100, 128), (22050, 127)]


def _iso_clips(bad):
    clean = _pcm(2, N_ISO)
    dirty = clean.copy()
    dirty[1, [2048 * t for t in BAD_FRAMES]] = bad
    return clean, dirty


def _assert_isolated(clean_out, dirty_out, must_be_nan):
    """[2, rows, 13]: the bad frames of clip 1 are non-finite in every row, all else is bit-equal to the clean run."""
    T = 1 + N_ISO // HOP_ISO
    assert clean_out.shape == dirty_out.shape and clean_out.shape[0] == 2 and clean_out.shape[-1] == T
    assert np.isfinite(clean_out).all()
    good = np.setdiff1d(np.arange(T), BAD_FRAMES)
    assert np.array_equal(dirty_out[0], clean_out[0]), "clip 0 changed"
    same = dirty_out[1][..., good] == clean_out[1][..., good]
    assert same.all(), ("clean frames of clip 1 changed", sorted(set(good[np.nonzero(~same)[-1]])))
    hit = dirty_out[1][..., BAD_FRAMES]
    assert (np.isnan(hit) if must_be_nan else ~np.isfinite(hit)).all()


# A NaN sample makes every power bin of its frame NaN, and every mel band (each sums at least one 8-bin step) and the
# centroid / bandwidth sums with them.  An Inf sample makes each power bin Inf or NaN (Inf - Inf in the butterflies);
# a band over such bins is Inf or NaN (0 * Inf under its zero weights), so there the test asks for "not finite";
# centroid / bandwidth normalise by the (Inf or NaN) total in float32, Inf / Inf = NaN, and stay NaN.
@pytest.mark.parametrize("grid", [None, 8])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("sr,n_mels", MEL_PLANS)
def test_nonfinite_sample_stays_in_its_frames_mel(cuda, sr, n_mels, bad, grid):
    clean, dirty = _iso_clips(bad)
    with stft_grid(grid):
        ref = hlmc_amd.melspectrogram(clean, sr=sr, n_mels=n_mels, hop_length=HOP_ISO)
        got = hlmc_amd.melspectrogram(dirty, sr=sr, n_mels=n_mels, hop_length=HOP_ISO)
    _assert_isolated(ref, got, must_be_nan=np.isnan(bad))


@pytest.mark.parametrize("grid", [None, 8])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_nonfinite_sample_stays_in_its_frames_spectral(cuda, bad, grid):
    clean, dirty = _iso_clips(bad)
    with stft_grid(grid):
        ref = hlmc_amd.extract_spectral_features(clean, hop_length=HOP_ISO)
        got = hlmc_amd.extract_spectral_features(dirty, hop_length=HOP_ISO)
    for k in ("spectral_centroid", "spectral_bandwidth"):
        _assert_isolated(ref[k], got[k], must_be_nan=True)
    # rolloff compares against a NaN threshold (librosa's own answer there is 0 Hz, no NaN) and zcr counts sign bits:
    # neither has to be NaN in the bad frames, but every other frame must not move; rms of the frame is NaN / Inf
    good = np.setdiff1d(np.arange(13), BAD_FRAMES)
    for k in ("spectral_rolloff", "zcr", "rms"):
        assert np.array_equal(got[k][0], ref[k][0]), k
        assert np.array_equal(got[k][1][..., good], ref[k][1][..., good]), k
    assert not np.isfinite(got["rms"][1][..., BAD_FRAMES]).any()


# ------------------------------------------------------------------------------------------- 3. tuning_kernel, T > 1024
def _late_tones(n):
    """Silence up to frame 1023, then (frames 1024..1030 only) three loud partials tuned +0.30 semitones and six
    quieter ones (0.4 x the amplitude: 0.16 x the power, above piptrack's 0.1 x max threshold) tuned -0.20.
    estimate_tuning keeps the peaks at or above the median magnitude: the loud ones and about one quiet one per
    frame, so the histogram peaks at +0.29.  A count loop that stops at frame 1023 sees no peak at all, takes the
    threshold 0, keeps all nine per frame, and the quiet majority moves the estimate to -0.20."""
    y = np.zeros((1, n), np.float32)
    start = 512 * 1023 + 1024                      # first sample past frame 1023's window
    t = np.arange(n - start) / 22050.0
    tone = lambda k, det: np.sin(2 * np.pi * 440.0 * 2.0 ** ((k + det) / 12) * t + k)
    y[0, start:] = (0.2 * sum(tone(k, 0.30) for k in (15, 20, 25)) +
                    0.08 * sum(tone(k, -0.20) for k in (12, 17, 22, 27, 32, 34))).astype(np.float32)
    return y


@pytest.mark.parametrize("kind", ["synthetic", "late_tones"])
def test_chroma_more_frames_than_the_tuning_block(cuda, kind):
    """tuning_kernel runs 1024 threads per clip: T = 1031 is the first size class at which its per-frame count loop
    takes a second trip.  `late_tones` puts every peak into the frames of that second trip."""
    n = 512 * 1030
    y = _pcm(1, n) if kind == "synthetic" else _late_tones(n)
    assert MO.n_frames(n) == 1031
    if kind == "late_tones":
        assert SO.estimate_tuning(MO.power_spectrogram(y[0])) > 0.25   # the signal does what its docstring says
    c, tun = hlmc_amd.chroma_stft(y, return_tuning=True)
    ref, rt = SO.chroma_stft(y[0])
    assert c.shape == (1, 12, 1031) and tun[0] == rt, (tun[0], rt)
    np.testing.assert_allclose(c[0], ref, rtol=1e-4, atol=1e-6)
