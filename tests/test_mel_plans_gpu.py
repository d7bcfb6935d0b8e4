"""The mel front end at plans other than the default (sr 22050, n_mels 128, fmin 0, fmax sr / 2).

The plan decides which instance of stft_mel0_kernel runs and how its band table looks (csrc/features.hip
plan_create: lane l owns the bands l and n_mels-1-l; C = the largest chunk count of a lane; the chunk-transposed
weights live in LDS up to 16 KB, in global memory above that).  For n_fft = 2048:

    sr     n_mels  fmin, fmax   C    weights   highest power-row float a band reads
    22050  128     default      16   LDS       1023
    22050  127     default      16   LDS       1023    odd n_mels: the middle lane has one band (m0 == m1)
    22050   64     default      30   global    1023    lanes 32..63 have no band
    22050   40     default      44   global    1023
    22050    2     default     312   global    1023    (the library's table: 1031, a 1.5e-19 residue at bin 1024)
    22050    1     default     256   global    1023    one lane, one band over every bin
    22050  128     20, 8000     12   LDS        747
     8000  128     default      14   LDS       1023
    16000   80     default      24   global    1027    reads the row's zero padding
    44100  128     default      20   global    1031    reads the row's zero padding to its end
    48000  128     default      20   global    1031

Every check compares against oracle/mel_oracle.py on the same float32 samples at the tolerances test_features_gpu.py
states for the default plan (float32 STFT vs the oracle's float64 one): power rtol 2e-4 + 1e-6 max, dB 0.05 overall
and 2e-3 above -60 dB, MFCC 0.05 + 1e-3.  Clips: B = 2, an even length (8-byte sample-pair loads) and an odd one
(4-byte loads); hop 441 (odd: 4-byte loads whatever the length) and 2048 at (22050, 64)."""
import functools

import numpy as np
import pytest

import hlmc_amd
from oracle import mel_oracle as MO

pytestmark = pytest.mark.gpu

# (sr, n_mels, fmin, fmax)
PLANS = [(22050, 128, 0.0, None), (22050, 127, 0.0, None), (22050, 64, 0.0, None), (22050, 40, 0.0, None),
         (22050, 2, 0.0, None), (22050, 1, 0.0, None), (22050, 128, 20.0, 8000.0), (8000, 128, 0.0, None),
         (16000, 80, 0.0, None), (44100, 128, 0.0, None), (48000, 128, 0.0, None)]
DEFAULT_BAND = [p for p in PLANS if p[2] == 0.0 and p[3] is None]   # extract_mel_spectrogram / mfcc take no fmin / fmax
LENGTHS = [22050, 22050 + 17]
# plan x hop: every plan at the default hop, (22050, 64) also at an odd hop and at hop = n_fft
CASES = [(p, 512) for p in PLANS] + [((22050, 64, 0.0, None), h) for h in (441, 2048)]
CASES_DEFAULT_BAND = [(p, h) for p, h in CASES if p in DEFAULT_BAND]


def _id(case):
    (sr, n_mels, fmin, fmax), hop = case
    return f"sr{sr}-m{n_mels}" + (f"-f{fmin:g}-{fmax:g}" if fmax else "") + (f"-hop{hop}" if hop != 512 else "")


@functools.lru_cache(maxsize=None)
def _pcm(n):
    return MO.synthetic_pcm(2, n, seed=n % 97)   # shared by the cases of one length; no test writes to it


@functools.lru_cache(maxsize=None)
def _power(n, hop):
    S = MO.power_spectrogram(_pcm(n), 2048, hop)     # float32 [2, 1025, T]
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _mel_ref(plan, n, hop):
    sr, n_mels, fmin, fmax = plan
    fb = MO.mel_filterbank(sr, 2048, n_mels, fmin, fmax)
    mel = np.einsum("...ft,mf->...mt", _power(n, hop), fb, optimize=True).astype(np.float32)
    mel.setflags(write=False)
    return mel


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: _id((p, 512)))
def test_filterbank(cuda, plan):
    sr, n_mels, fmin, fmax = plan
    got = hlmc_amd.mel_filterbank(sr=sr, n_mels=n_mels, fmin=fmin, fmax=fmax)
    np.testing.assert_allclose(got, MO.mel_filterbank(sr, 2048, n_mels, fmin, fmax), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mel_power(cuda, case, n):
    (sr, n_mels, fmin, fmax), hop = case
    got = hlmc_amd.melspectrogram(_pcm(n), sr=sr, hop_length=hop, n_mels=n_mels, fmin=fmin, fmax=fmax)
    ref = _mel_ref(case[0], n, hop)
    assert got.shape == ref.shape == (2, n_mels, 1 + n // hop)
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-6 * ref.max())


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("case", CASES_DEFAULT_BAND, ids=_id)
def test_mel_db(cuda, case, n):
    (sr, n_mels, _, _), hop = case
    got = hlmc_amd.extract_mel_spectrogram(_pcm(n), sr=sr, n_mels=n_mels, hop_length=hop)
    ref = np.stack([MO.power_to_db(m, ref=np.max) for m in _mel_ref(case[0], n, hop)])
    assert got.shape == ref.shape
    d = np.abs(got - ref)
    hi = ref > -60
    print(f"{_id(case)} n={n}: max |dB| {d.max():.2e}, above -60 dB {d[hi].max():.2e}")
    np.testing.assert_allclose(got, ref, atol=0.05)
    assert d[hi].max() < 2e-3


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("case", CASES_DEFAULT_BAND, ids=_id)
def test_mfcc(cuda, case, n):
    """n_mfcc = 1 (the DC row alone), min(40, n_mels) (the reference's 40) and n_mels (the whole DCT)."""
    (sr, n_mels, _, _), hop = case
    mel = _mel_ref(case[0], n, hop)
    db = np.stack([MO.power_to_db(m, ref=1.0) for m in mel]).astype(np.float64)
    for n_mfcc in sorted({1, min(40, n_mels), n_mels}):
        got = hlmc_amd.mfcc(_pcm(n), sr=sr, n_mfcc=n_mfcc, hop_length=hop, n_mels=n_mels)
        ref = np.einsum("km,bmt->bkt", MO.dct_ortho_matrix(n_mels, n_mfcc), db).astype(np.float32)
        assert got.shape == ref.shape == (2, n_mfcc, 1 + n // hop)
        e = np.abs(got - ref) - (0.05 + 1e-3 * np.abs(ref))
        print(f"{_id(case)} n={n} n_mfcc={n_mfcc}: max |d| {np.abs(got - ref).max():.2e}, over tolerance {e.max():.2e}")
        np.testing.assert_allclose(got, ref, atol=0.05, rtol=1e-3, err_msg=f"n_mfcc={n_mfcc}")
