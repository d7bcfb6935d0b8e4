"""The ops that carve a caller's workspace stay inside the bytes their *_workspace query states: each op below runs on
an allocation of exactly that many bytes followed by a guard region filled with a sentinel.  Afterwards the guard must
be untouched and the outputs complete: pre-filled with NaN, they carry a spare element that stays NaN, hold no NaN
elsewhere, and equal bit for bit what the package's own wrapper (which allocates its own workspace) returns.

Mel ops (csrc/features.hip): hlmc_melspectrogram, hlmc_mel_db, hlmc_mel_db_zscore (f32 and bf16), hlmc_mfcc and
hlmc_chroma_stft at B = 3 and 65 (4 B rounds to 256 and to 512 bytes), clip lengths 8192 and 8191 (the pair-load and
the single-load STFT variants) and the plans n_mels = 128 and 40 (at B = 3 and n_mels = 40 the mel power's size is no
multiple of 256).  K-Means (csrc/kmeans.hip): hlmc_km_sums_batch on its partition path (n = 4097), R = 3."""
import functools

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from hlmc_amd import features as F
from oracle import kmeans_oracle as KO

pytestmark = pytest.mark.gpu

GUARD = 4096       # bytes behind the workspace
SENT = 0xA5
KEEP = 20          # frames kept by the dB ops: a multiple of 4 above T = 17 / 16, so the clip-minimum padding is read


def _ws(nbytes):
    return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")


def _guard_untouched(ws, nbytes):
    torch.cuda.synchronize()
    return ws.numel() == nbytes + GUARD and bool((ws[nbytes:] == SENT).all())


def _nan(n, dtype=torch.float32):
    return torch.full((n + 1,), float("nan"), dtype=dtype, device="cuda")


def _complete(out, n):
    """the n outputs are written (no NaN left) and the spare element behind them is not"""
    o = out.float() if out.dtype == torch.bfloat16 else out
    return bool(torch.isnan(o[n:]).all()) and not bool(torch.isnan(o[:n]).any())


@functools.lru_cache(maxsize=None)
def _pcm(B, n):
    g = torch.Generator().manual_seed(1000 * B + n)
    return (0.3 * torch.randn(B, n, generator=g)).to("cuda")          # read-only: shared by the cases of one shape


@pytest.mark.parametrize("n_mels", [128, 40])
@pytest.mark.parametrize("n", [8192, 8191])
@pytest.mark.parametrize("B", [3, 65])
def test_mel_ops_stay_inside_their_workspace(cuda, B, n, n_mels):
    lib = L.lib()
    x = _pcm(B, n)
    p = F._plan(22050, 2048, 512, n_mels)
    T = int(lib.hlmc_mel_frames(p, n))
    assert T == 1 + n // 512 and T < KEEP
    nb = int(lib.hlmc_mel_workspace(p, B, n))
    assert nb >= B * n_mels * T * 4 + 8 * B
    s = L.stream()

    ws, out = _ws(nb), _nan(B * n_mels * T)
    L.check(lib.hlmc_melspectrogram(p, s, x.data_ptr(), B, n, out.data_ptr(), ws.data_ptr()), "hlmc_melspectrogram")
    assert _guard_untouched(ws, nb) and _complete(out, B * n_mels * T)
    assert torch.equal(out[:-1].view(B, n_mels, T), hlmc_amd.melspectrogram(x, n_mels=n_mels))

    def mel_db(ws):
        out = _nan(B * n_mels * KEEP)
        L.check(lib.hlmc_mel_db(p, s, x.data_ptr(), B, n, KEEP, 1e-10, 80.0, out.data_ptr(), ws.data_ptr()), "hlmc_mel_db")
        return out

    ws = _ws(nb)
    db = mel_db(ws)
    assert _guard_untouched(ws, nb) and _complete(db, B * n_mels * KEEP)
    again = mel_db(ws)                                  # the same workspace, as the first call left it
    roomy = mel_db(_ws(2 * nb + 1024))
    assert _guard_untouched(ws, nb)
    assert torch.equal(db.view(torch.int32)[:-1], again.view(torch.int32)[:-1])
    assert torch.equal(db.view(torch.int32)[:-1], roomy.view(torch.int32)[:-1])
    want = hlmc_amd.extract_mel_spectrogram(x, n_mels=n_mels, fixed_time_steps=KEEP)
    assert torch.equal(db[:-1].view(B, n_mels, KEEP), want)

    rng = np.random.default_rng(B + n + n_mels)
    mean = torch.from_numpy(rng.normal(-40.0, 5.0, n_mels * KEEP)).to("cuda")
    scale = torch.from_numpy(rng.uniform(0.5, 9.0, n_mels * KEEP)).to("cuda")
    zs = {}
    for dtype, code in ((torch.float32, L.HLMC_F32), (torch.bfloat16, L.HLMC_BF16)):
        ws, out = _ws(nb), _nan(B * n_mels * KEEP, dtype)
        L.check(lib.hlmc_mel_db_zscore(p, s, x.data_ptr(), B, n, KEEP, 1e-10, 80.0, mean.data_ptr(), scale.data_ptr(),
                                       code, out.data_ptr(), ws.data_ptr()), "hlmc_mel_db_zscore")
        assert _guard_untouched(ws, nb) and _complete(out, B * n_mels * KEEP), dtype
        zs[dtype] = out[:-1].clone()
    # the transform of hlmc_zscore_apply on the dB output above (include/hlmc.h: bit-identical to that pair)
    a = (db[:-1].double().view(B, -1) - mean).float()
    z = (a.double() / scale).float().reshape(-1)
    assert torch.equal(zs[torch.float32], z) and torch.equal(zs[torch.bfloat16], z.to(torch.bfloat16))

    n_mfcc = 20
    ws, out = _ws(nb), _nan(B * n_mfcc * T)
    L.check(lib.hlmc_mfcc(p, s, x.data_ptr(), B, n, n_mfcc, out.data_ptr(), ws.data_ptr()), "hlmc_mfcc")
    assert _guard_untouched(ws, nb) and _complete(out, B * n_mfcc * T)
    assert torch.equal(out[:-1].view(B, n_mfcc, T), hlmc_amd.mfcc(x, n_mfcc=n_mfcc, n_mels=n_mels))

    cb = int(lib.hlmc_chroma_workspace(p, B, n))
    ws, out, tun = _ws(cb), _nan(B * 12 * T), _nan(B, torch.float64)
    L.check(lib.hlmc_chroma_stft(p, s, x.data_ptr(), B, n, out.data_ptr(), tun.data_ptr(), ws.data_ptr()),
            "hlmc_chroma_stft")
    assert _guard_untouched(ws, cb) and _complete(out, B * 12 * T) and _complete(tun, B)
    if n_mels == 128:     # the wrapper's plan
        c, t = hlmc_amd.chroma_stft(x, return_tuning=True)
        assert torch.equal(out[:-1].view(B, 12, T), c) and torch.equal(tun[:-1], t)


def test_km_sums_batch_partition_stays_inside_its_workspace(cuda):
    n, d, k, R = 4097, 65, 5, 3
    rng = np.random.default_rng(n + d + k)
    X = rng.normal(0, 2.0, (n, d)).astype(np.float32)
    lab = rng.integers(0, k, (R, n)).astype(np.int32)
    Xd, ld = torch.from_numpy(X).to("cuda"), torch.from_numpy(lab).to("cuda")
    nb = R * int(L.lib().hlmc_km_sums_workspace(n, k))
    ws, sums, w = _ws(nb), _nan(R * k * d), _nan(R * k)
    L.check(L.lib().hlmc_km_sums_batch(L.stream(), Xd.data_ptr(), n, d, ld.data_ptr(), k, R, (1 << R) - 1,
                                       sums.data_ptr(), w.data_ptr(), ws.data_ptr(), nb), "hlmc_km_sums_batch")
    assert _guard_untouched(ws, nb) and _complete(sums, R * k * d) and _complete(w, R * k)
    sums, w = sums[:-1].view(R, k, d).cpu().numpy(), w[:-1].view(R, k).cpu().numpy()
    for r in range(R):
        rs, rw = KO.cluster_sums_f32(X, lab[r], k)
        np.testing.assert_array_equal(sums[r].view(np.int32), rs.view(np.int32), err_msg=f"sums of restart {r}")
        np.testing.assert_array_equal(w[r].view(np.int32), rw.view(np.int32), err_msg=f"weights of restart {r}")
