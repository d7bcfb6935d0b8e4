"""hlmc_silhouette, hlmc_cluster_scores and the scaler / pooling / dB entry points validate their arguments on the
host, ahead of any launch: every case below passes placeholder pointers, so it must come back with status -1
(HLMC_EINVAL) and the matching hlmc_last_error() without a device being touched (csrc/metrics.hip, the tail of
csrc/features.hip).  StandardScaler.transform checks the feature count before anything is moved to the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L

ONE = C.c_void_p(256)          # non-null placeholder: validation fails before anything is dereferenced


def _reject(call, base, cases):
    lib = L.lib()
    for change, msg in cases:
        a = dict(base)
        a.update(change)
        st = call(lib, a)
        assert st == -1, (change, st, lib.hlmc_last_error())
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())


def _nulls(msg, *names):
    return [({n: None}, msg) for n in names]


def test_silhouette_rejects_bad_arguments():
    lib = L.lib()
    n, k = 100, 5
    ws = int(lib.hlmc_silhouette_workspace(n, k))
    assert ws == (n * k * 8 + 255) // 256 * 256 + 256 + 512 * 8      # S | counts (256-byte units) | 512 block partials
    _reject(lambda lib, a: lib.hlmc_silhouette(None, a["X"], a["n"], a["d"], a["labels"], a["k"], a["samples"],
                                               a["score"], a["ws"], a["ws_bytes"]),
            dict(X=ONE, n=n, d=8, labels=ONE, k=k, samples=ONE, score=ONE, ws=ONE, ws_bytes=ws),
            _nulls(b"NULL argument", "X", "labels", "score", "ws") + [
                (dict(n=1), b"need n >= 2"), (dict(n=0), b"need n >= 2"), (dict(n=-3), b"need n >= 2"),
                (dict(d=0), b"1 <= d <= 128"), (dict(d=-1), b"1 <= d <= 128"), (dict(d=129), b"1 <= d <= 128"),
                (dict(k=1), b"[2, n - 1]"), (dict(k=0), b"[2, n - 1]"), (dict(k=n), b"[2, n - 1]"),
                (dict(k=n + 1), b"[2, n - 1]"),
                (dict(ws_bytes=ws - 1), b"workspace too small"),          # one byte short
                (dict(ws_bytes=0), b"workspace too small"), (dict(ws_bytes=-1), b"workspace too small"),
                (dict(k=k + 60, ws_bytes=ws), b"workspace too small")])   # sized for another k


def test_cluster_scores_rejects_bad_arguments():
    lib = L.lib()
    n, k, d = 2000, 5, 8
    ws = int(lib.hlmc_cluster_scores_workspace(k, d))
    assert ws == (64 * k * d + 64 * k * 2 + k * d + d) * 8 + 256 + k * 8   # part | part2 | cent | mean | counts | intra
    big = int(lib.hlmc_cluster_scores_workspace(1025, 4097))
    _reject(lambda lib, a: lib.hlmc_cluster_scores(None, a["X"], a["n"], a["d"], a["labels"], a["k"], a["out"], a["ws"],
                                                   a["ws_bytes"]),
            dict(X=ONE, n=n, d=d, labels=ONE, k=k, out=ONE, ws=ONE, ws_bytes=ws),
            _nulls(b"NULL argument", "X", "labels", "out", "ws") + [
                (dict(n=1), b"need n >= 2"), (dict(n=0), b"need n >= 2"),
                (dict(d=0), b"1 <= d <= 4096"), (dict(d=4097, ws_bytes=big), b"1 <= d <= 4096"),
                (dict(k=1), b"[2, n - 1]"), (dict(k=n, ws_bytes=big), b"[2, n - 1]"),
                (dict(k=1025, ws_bytes=big), b"k too large"),
                (dict(ws_bytes=ws - 1), b"workspace too small"), (dict(ws_bytes=-1), b"workspace too small"),
                (dict(d=d + 1), b"workspace too small")])


def test_scaler_pool_and_db_entry_points_reject_bad_arguments():
    sizes = [(dict(n=0), b"arguments"), (dict(n=-1), b"arguments"), (dict(cols=0), b"arguments"),
             (dict(cols=-7), b"arguments")]
    base = dict(x=ONE, n=10, cols=4, mean=ONE, sd=ONE, out=ONE, o1=ONE, ws=ONE)
    _reject(lambda lib, a: lib.hlmc_row_mean_std(None, a["x"], a["n"], a["cols"], a["mean"], a["sd"]),
            base, _nulls(b"row_mean_std arguments", "x", "mean", "sd") + sizes)
    _reject(lambda lib, a: lib.hlmc_colstats_sum(None, a["x"], a["n"], a["cols"], a["out"], a["ws"]),
            base, _nulls(b"colstats arguments", "x", "out", "ws") + sizes)
    _reject(lambda lib, a: lib.hlmc_colstats_centered(None, a["x"], a["n"], a["cols"], a["mean"], a["out"], a["o1"],
                                                      a["ws"]),
            base, _nulls(b"colstats arguments", "x", "out", "ws") + _nulls(b"mean and m2 required", "mean", "o1") + sizes)
    _reject(lambda lib, a: lib.hlmc_zscore_apply(None, a["x"], a["n"], a["cols"], a["mean"], a["sd"], 0, a["out"]),
            base, _nulls(b"zscore arguments", "x", "mean", "sd", "out") + sizes)
    _reject(lambda lib, a: lib.hlmc_power_to_db(None, a["x"], a["n"], a["cols"], 1, 0.0, 1e-10, 80.0, a["out"], a["ws"]),
            base, _nulls(b"power_to_db arguments", "x", "out", "ws") + sizes + [
                (dict(n=65536), b"power_to_db arguments"), (dict(cols=1 << 31), b"power_to_db arguments")])
    assert L.lib().hlmc_colstats_workspace(16385, 513) == 2 * 256 * 513 * 8
    assert L.lib().hlmc_colstats_workspace(1, 1) == 16 and L.lib().hlmc_colstats_workspace(129, 3) == 2 * 2 * 3 * 8


@pytest.mark.parametrize("shape", [(10, 6), (10, 4), (10, 2, 3), (10,), (3, 5, 2)])
def test_standard_scaler_transform_checks_feature_count_before_the_device(shape):
    """A scaler fitted on 5 columns (attributes built by hand: no fit, no device) raises sklearn's ValueError for any
    other feature count, numpy or tensor input, before the input is converted or moved: with more columns than were
    fitted, zscore_kernel would read mean_ / scale_ out of bounds."""
    sc = hlmc_amd.StandardScaler()
    sc.n_features_in_ = 5
    sc.mean_d = sc.scale_d = None          # touching them would raise AttributeError, not ValueError
    X = np.zeros(shape, dtype=np.float32)
    for x in (X, torch.from_numpy(X), X.tolist()):
        with pytest.raises(ValueError, match="features|dimensions"):
            sc.transform(x)
