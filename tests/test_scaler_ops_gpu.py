"""Op-level parity of the tail of csrc/features.hip -- the StandardScaler passes (hlmc_colstats_sum / _centered,
hlmc_zscore_apply), the mean / std pooling (hlmc_row_mean_std) and the generic librosa.power_to_db
(hlmc_power_to_db) -- against oracle/scaler_oracle.py: exact sums and float64 restatements with bounds counted from the
roundings the kernels' number formats allow (tests/test_oracle_cpu.py pins the oracle to live sklearn and holds the
restatements inside the same bounds on the same inputs).  Shapes sit on the edges the code has: the row chunking
clamp(n / 64, 1, 256) with its empty trailing chunks, the 256-thread column blocks, the grid cap of 8192 x 256 threads
(grid-stride loop and its column index), part-filled 4-row blocks and part-filled waves in the pooling kernel.

Outputs are pre-filled with NaN and carry a spare element.  Every test prints its worst |err| / bound as
"RATIO <quantity> <case> <value>"."""
import numpy as np
import pytest
import torch
from sklearn.preprocessing import StandardScaler as SkScaler

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import scaler_oracle as SO
from tests import scaler_cases as SC

pytestmark = pytest.mark.gpu


def _nan64(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    assert (err[bound == 0] == 0).all(), "non-zero error where the reference is exact"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("n,cols", SC.COLSTATS_CASES, ids=SC.COLSTATS_IDS)
def test_colstats_passes_within_exact_sum_bounds_and_fit_matches_sklearn(cuda, n, cols):
    """hlmc_colstats_sum and hlmc_colstats_centered, on a workspace of exactly hlmc_colstats_workspace bytes followed
    by a NaN guard, within the exact-sum bounds of the oracle (n 2^-53 sum|terms|; 0 for a column sum whose float64
    partial sums are exact in any order, which then has to come out bit-equal); then StandardScaler.fit on the same input
    against live sklearn (mean_ 1e-14, var_ / scale_ 1e-10), a constant 0.1 column and a mean-1e4 / std-1e-2 column
    included."""
    X = SC.colstats_input(n, cols)
    Xd = torch.as_tensor(X, device="cuda")
    lib = L.lib()
    nbytes = int(lib.hlmc_colstats_workspace(n, cols))
    assert nbytes % 8 == 0 and nbytes == 2 * max(1, min(256, n // 64)) * cols * 8
    ws = _nan64(nbytes // 8 + 4)
    s, corr, m2 = _nan64(cols + 1), _nan64(cols + 1), _nan64(cols + 1)
    L.check(lib.hlmc_colstats_sum(L.stream(), Xd.data_ptr(), n, cols, s.data_ptr(), ws.data_ptr()), "hlmc_colstats_sum")
    torch.cuda.synchronize()
    assert torch.isnan(ws[nbytes // 8:]).all(), "hlmc_colstats_sum wrote past hlmc_colstats_workspace bytes"
    s_ref, s_b = SO.col_sums(X)
    got_s = s.cpu().numpy()
    assert np.isnan(got_s[cols]) and not np.isnan(got_s[:cols]).any()
    mean = torch.as_tensor(got_s[:cols] / float(n), device="cuda")
    L.check(lib.hlmc_colstats_centered(L.stream(), Xd.data_ptr(), n, cols, mean.data_ptr(), corr.data_ptr(),
                                       m2.data_ptr(), ws.data_ptr()), "hlmc_colstats_centered")
    torch.cuda.synchronize()
    assert torch.isnan(ws[nbytes // 8:]).all(), "hlmc_colstats_centered wrote past hlmc_colstats_workspace bytes"
    got_c, got_m = corr.cpu().numpy(), m2.cpu().numpy()
    assert np.isnan(got_c[cols]) and np.isnan(got_m[cols])
    assert not np.isnan(got_c[:cols]).any() and not np.isnan(got_m[:cols]).any()
    c_ref, c_b, m_ref, m_b = SO.col_centered(X, got_s[:cols] / float(n))
    r = (_ratio(np.abs(got_s[:cols] - s_ref), s_b), _ratio(np.abs(got_c[:cols] - c_ref), c_b),
         _ratio(np.abs(got_m[:cols] - m_ref), m_b))
    print(f"RATIO colsum n{n}_c{cols} {r[0]:.4f}\nRATIO corr n{n}_c{cols} {r[1]:.4f}\nRATIO m2 n{n}_c{cols} {r[2]:.4f}")
    assert r[0] <= 1.0 and r[1] <= 1.0 and r[2] <= 1.0, r
    sk = SkScaler().fit(X)
    ours = hlmc_amd.StandardScaler().fit(X)
    np.testing.assert_allclose(ours.mean_, sk.mean_, rtol=1e-14)
    np.testing.assert_allclose(ours.var_, sk.var_, rtol=1e-10)
    np.testing.assert_allclose(ours.scale_, sk.scale_, rtol=1e-10)
    assert ours.n_samples_seen_ == n and ours.n_features_in_ == cols
    if cols > SC.SHIFTED_COL:
        assert ours.scale_[SC.CONST_COL] == 1.0


@pytest.mark.parametrize("shape", SC.TRANSFORM_SHAPES, ids=SC.TRANSFORM_IDS)
def test_standard_scaler_transform_bit_equal_in_every_element(cuda, shape):
    """transform == f32(f32(x - mean) / scale) evaluated in float64 (include/hlmc.h) in EVERY element, with the
    scaler's own mean_ / scale_; the bf16 output is torch's rounding of that; a wrong feature count raises."""
    X = SC.transform_input(shape)
    sc = hlmc_amd.StandardScaler().fit(X)
    want = SO.zscore(X.reshape(shape[0], -1), sc.mean_, sc.scale_).reshape(shape)
    got = sc.transform(X)
    assert got.shape == X.shape and got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    got_t = sc.transform(torch.as_tensor(X, device="cuda"))
    assert torch.equal(got_t.cpu(), torch.from_numpy(want))
    bf = sc.transform(torch.as_tensor(X, device="cuda"), out_dtype=torch.bfloat16)
    assert bf.dtype == torch.bfloat16 and tuple(bf.shape) == tuple(shape)
    assert torch.equal(bf.cpu(), torch.from_numpy(want).to(torch.bfloat16))
    assert np.array_equal(sc.fit_transform(X), want)
    with pytest.raises(ValueError, match="features"):
        sc.transform(X.reshape(shape[0], -1)[:, :-1])
    with pytest.raises(ValueError, match="features"):
        sc.transform(np.concatenate([X.reshape(shape[0], -1)] * 2, axis=1))


@pytest.mark.parametrize("kind", list(SC.POOL_KINDS))
@pytest.mark.parametrize("rows", SC.POOL_ROWS)
def test_mean_std_pool_within_bound(cuda, rows, kind):
    """hlmc_row_mean_std (a float64 two-pass, one float32 rounding) within 2^-24 |ref| + cols 2^-52 mean|x| of the
    exact row mean / std, for cols = 1, 63, 64, 65 and 300, on values around -30 +- 10 and around 0 +- 1."""
    worst = [0.0, 0.0]
    for cols in SC.POOL_COLS:
        x = SC.pool_input(rows, cols, kind)
        m, mb, sd, sb = SO.row_mean_std(x)
        got = hlmc_amd.mean_std_pool(x)
        assert got.shape == (2 * rows,) and got.dtype == np.float32 and not np.isnan(got).any()
        got3 = hlmc_amd.mean_std_pool(torch.as_tensor(np.stack([x, x]), device="cuda")).cpu().numpy()
        assert got3.shape == (2, 2 * rows) and np.array_equal(got3[0], got) and np.array_equal(got3[1], got)
        rm, rs = _ratio(np.abs(got[:rows] - m), mb), _ratio(np.abs(got[rows:] - sd), sb)
        assert rm <= 1.0 and rs <= 1.0, (cols, rm, rs)
        if cols == 1:
            assert (got[rows:] == 0.0).all() and np.array_equal(got[:rows], x[:, 0])
        worst = [max(worst[0], rm), max(worst[1], rs)]
    print(f"RATIO rowmean r{rows}_{kind} {worst[0]:.4f}\nRATIO rowstd r{rows}_{kind} {worst[1]:.4f}")


def test_row_mean_std_leaves_the_rows_past_the_end_alone(cuda):
    """rows = 5: the second block's waves 1 .. 3 own no row and must not write (the spare elements stay NaN)."""
    x = SC.pool_input(5, 65, "db_like")
    xd = torch.as_tensor(x, device="cuda")
    mean = torch.full((8,), float("nan"), device="cuda")
    sd = torch.full((8,), float("nan"), device="cuda")
    L.check(L.lib().hlmc_row_mean_std(L.stream(), xd.data_ptr(), 5, 65, mean.data_ptr(), sd.data_ptr()),
            "hlmc_row_mean_std")
    torch.cuda.synchronize()
    assert torch.isnan(mean[5:]).all() and torch.isnan(sd[5:]).all()
    assert not torch.isnan(mean[:5]).any() and not torch.isnan(sd[:5]).any()


@pytest.mark.parametrize("case", SC.DB_CASES, ids=SC.DB_IDS)
def test_power_to_db_within_bound(cuda, case):
    """hlmc_power_to_db against the float64 librosa.power_to_db per clip within
    2^-24 ((L + 1)(|db_S| + |db_ref|) + |out|), L = 2 ulp assumed for the device log10f: ref = np.max and ref = 1.0,
    top_db 80 and None, a clip of zeros only, values below amin and exact zeros, and 2 100 003 elements (past the grid
    cap).  Elements that are below the floor whatever the roundings equal max - top_db of the same call exactly."""
    name, B, F, T, zero_clip, ref_max, top_db = case
    S = SC.db_input(B, F, T, seed=B + F + T, zero_clip=zero_clip)
    arg = S[0] if B == 1 else S                       # one clip [F, T], or a batch [B, F, T]
    got = hlmc_amd.power_to_db(arg, ref=np.max if ref_max else 1.0, top_db=top_db)
    assert got.shape == arg.shape and got.dtype == np.float32 and not np.isnan(got).any()
    got = got.reshape(B, -1)
    ref, bound, clamped = SO.power_to_db(S.reshape(B, -1), ref_max=ref_max, top_db=top_db)
    r = _ratio(np.abs(got - ref), bound)
    print(f"RATIO dB {name} {r:.4f}")
    assert r <= 1.0, r
    if zero_clip is not None:
        assert (got[zero_clip] == got[zero_clip][0]).all()
    if top_db is not None:
        for b in range(B):
            assert (got[b][clamped[b]] == got[b].max() - np.float32(top_db)).all()
            assert got[b].min() >= got[b].max() - np.float32(top_db)
        assert clamped.any()
    on_dev = hlmc_amd.power_to_db(torch.as_tensor(arg, device="cuda"), ref=np.max if ref_max else 1.0, top_db=top_db)
    assert torch.equal(on_dev.cpu(), torch.from_numpy(got.reshape(arg.shape)))
