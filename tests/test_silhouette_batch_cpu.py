"""The batched silhouette without a GPU: the header, the library's exports and the ctypes table agree on the two new
symbols; hlmc_silhouette_batch_workspace grows as include/hlmc.h's layout says; every argument check of
hlmc_silhouette_batch comes back with HLMC_EINVAL and its message before any launch (placeholder pointers, as in
tests/test_metrics_args_cpu.py); the Python surface is exported; and a numpy restatement of the kernel's windowed
multi-labelling accumulation reproduces the per-labelling float32 restatement of the single kernel bit for bit."""
import ctypes as C
import re

import numpy as np

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import metrics_oracle as MT
from tests import silhouette_batch_cases as BC

ONE = C.c_void_p(256)          # non-null placeholder: validation fails before anything is dereferenced
NEW = ("hlmc_silhouette_batch_workspace", "hlmc_silhouette_batch")


def _ks(*ks):
    return (C.c_int32 * len(ks))(*ks)


def _r256(b):
    return (b + 255) // 256 * 256


def test_header_exports_and_ctypes_table_agree_on_the_new_symbols():
    src = open("include/hlmc.h").read()
    declared = set(re.findall(r"\b(hlmc_[A-Za-z0-9_]+)\s*\(", src))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
    assert re.search(r"int64_t hlmc_silhouette_batch_workspace\(int64_t n, const int32_t\* ks, int M\);", src)
    assert re.search(r"int hlmc_silhouette_batch\(void\* stream, const float\* X, int64_t n, int d, const int32_t\* labels, "
                     r"const int32_t\* ks, int M,\s+double\* samples, double\* scores, void\* ws, int64_t ws_bytes\);", src)
    assert lib.hlmc_silhouette_batch_workspace.restype is C.c_int64
    assert len(lib.hlmc_silhouette_batch.argtypes) == 11


def test_python_surface_is_exported():
    for name in ("silhouette_scores",):
        assert callable(getattr(hlmc_amd.metrics, name))
    assert callable(hlmc_amd.kmeans_k_sweep) and hlmc_amd.kmeans_k_sweep is hlmc_amd.cluster.kmeans_k_sweep
    assert hlmc_amd.silhouette_scores is hlmc_amd.metrics.silhouette_scores
    assert {"silhouette_scores", "kmeans_k_sweep"} <= set(hlmc_amd.__all__)
    assert "silhouette_scores" in hlmc_amd.__doc__ and "kmeans_k_sweep" in hlmc_amd.__doc__
    assert "silhouette_scores" in hlmc_amd.metrics.__doc__ and "kmeans_k_sweep" in hlmc_amd.cluster.__doc__


def test_workspace_grows_as_the_documented_layout():
    """S [n][K] f64 | counts [K] int32 (both in 256-byte units) | M x 512 f64 block partials; -1 outside the range."""
    lib = L.lib()
    for n, ks in ((100, (5,)), (100, (2, 3)), (203, BC.SWEEP_KS), (3, (2, 2)), (130, (2,) * BC.MAX_BATCH),
                  (100000, BC.SWEEP_KS), (5000, (4999, 2, 77))):
        K = sum(ks)
        want = _r256(8 * n * K) + _r256(4 * K) + len(ks) * 512 * 8
        assert lib.hlmc_silhouette_batch_workspace(n, _ks(*ks), len(ks)) == want, (n, ks)
    # one labelling: the single call's size
    assert lib.hlmc_silhouette_batch_workspace(100, _ks(5), 1) == lib.hlmc_silhouette_workspace(100, 5)
    for n, ks, m in ((100, None, 1), (100, _ks(5), 0), (100, _ks(*(2,) * 65), 65), (1, _ks(2), 1), (100, _ks(1), 1),
                     (100, _ks(5, 100), 2), (2 ** 40, _ks(2 ** 31 - 1), 1)):
        assert lib.hlmc_silhouette_batch_workspace(n, ks, m) == -1, (n, m)


def test_silhouette_batch_rejects_bad_arguments():
    lib = L.lib()
    n, ks = 100, (2, 3)
    ws = int(lib.hlmc_silhouette_batch_workspace(n, _ks(*ks), 2))
    base = dict(X=ONE, n=n, d=8, labels=ONE, ks=_ks(*ks), M=2, samples=ONE, scores=ONE, ws=ONE, ws_bytes=ws)
    big = 1 << 62
    cases = [({name: None}, b"NULL argument") for name in ("X", "labels", "ks", "scores", "ws")] + [
        (dict(n=1), b"need n >= 2"), (dict(n=0), b"need n >= 2"), (dict(n=-3), b"need n >= 2"),
        (dict(d=0), b"1 <= d <= 128"), (dict(d=-1), b"1 <= d <= 128"), (dict(d=129), b"1 <= d <= 128"),
        (dict(M=0), b"1 <= M <= 64"), (dict(M=-1), b"1 <= M <= 64"),
        (dict(M=65, ks=_ks(*(2,) * 65), ws_bytes=big), b"1 <= M <= 64"),
        (dict(ks=_ks(2, 1)), b"[2, n - 1]"), (dict(ks=_ks(0, 3)), b"[2, n - 1]"), (dict(ks=_ks(2, n)), b"[2, n - 1]"),
        (dict(ks=_ks(n + 1, 3)), b"[2, n - 1]"), (dict(ks=_ks(-4, 3)), b"[2, n - 1]"),
        (dict(ws_bytes=ws - 1), b"workspace too small"), (dict(ws_bytes=0), b"workspace too small"),
        (dict(ws_bytes=-1), b"workspace too small"),
        (dict(ks=_ks(2, 60)), b"workspace too small"),                        # sized for other labellings
        (dict(n=2 ** 40, ks=_ks(2 ** 31 - 1, 2), ws_bytes=big), b"overflows"),  # K n 8 >= 2^63
        (dict(n=2 ** 31, ks=_ks(*(2 ** 31 - 2,) * 64), M=64, ws_bytes=big), b"overflows"),   # K above int32
    ]
    for change, msg in cases:
        a = dict(base)
        a.update(change)
        st = lib.hlmc_silhouette_batch(None, a["X"], a["n"], a["d"], a["labels"], a["ks"], a["M"], a["samples"],
                                       a["scores"], a["ws"], a["ws_bytes"])
        assert st == -1, (change, st, lib.hlmc_last_error())
        assert msg in lib.hlmc_last_error(), (change, lib.hlmc_last_error())
    # samples alone may be NULL: with it NULL the checks still reach the next failing one, not "NULL argument"
    st = lib.hlmc_silhouette_batch(None, ONE, n, 8, ONE, _ks(*ks), 2, None, ONE, ONE, ws - 1)
    assert st == -1 and b"workspace too small" in lib.hlmc_last_error()


def _dist_f32(X):
    """The kernel's distance as oracle.metrics_oracle.silhouette_sums_f32 restates it: a sequential float32 sum of
    squared float32 differences, float32 square root."""
    X = np.asarray(X, dtype=np.float32)
    s2 = np.zeros((X.shape[0], X.shape[0]), dtype=np.float32)
    for c in range(X.shape[1]):
        e = X[:, c, None] - X[None, :, c]
        s2 = s2 + e * e
    return np.sqrt(s2).astype(np.float64)


def _windowed_sums(X, Y, ks, kw_max):
    """sil_sums_batch_kernel in numpy: windows [c0, c0 + kw) of the concatenated label space; per window the labellings
    that overlap it with their labels shifted into it (-1 outside); row i's four subs (sub = j % 4: every 4th j of each
    64-row tile) each add the distance of j, in j order, into the accumulator of every overlapping labelling that has j
    inside the window; the four subs are combined in order.  Returns S [n][K] and the windows' (c0, kw, m0, ml)."""
    n = X.shape[0]
    D = _dist_f32(X)
    off = BC.offsets(ks)
    K = int(off[-1])
    S = np.full((n, K), np.nan)
    windows = []
    for c0 in range(0, K, kw_max):
        kw = min(kw_max, K - c0)
        over = [m for m in range(len(ks)) if off[m + 1] > c0 and off[m] < c0 + kw]
        assert over == list(range(over[0], over[-1] + 1)) and len(over) <= kw // 2 + 1
        windows.append((c0, kw, over[0], len(over)))
        shifted = []
        for m in over:
            l = Y[m].astype(np.int64) + off[m] - c0
            shifted.append(np.where((l >= 0) & (l < kw), l, -1))
        acc = np.zeros((n, 4, kw))
        for j in range(n):
            for l in shifted:
                if l[j] >= 0:
                    acc[:, j % 4, l[j]] += D[:, j]
        v = np.zeros((n, kw))
        for u in range(4):
            v = v + acc[:, u, :]
        S[:, c0:c0 + kw] = v
    return S, windows


def test_windowed_accumulation_reproduces_the_single_restatement_bit_for_bit():
    """The identity argument on the k-sweep case at both window widths: each (row, sub, column) accumulator sees the
    same j sequence whatever the window and whichever other labellings share it, so each labelling's columns equal
    MT.silhouette_sums_f32 of that labelling alone.  The case has two windows and a labelling that straddles them."""
    for d in (16, 128):
        X, Y, ks = BC.case_input(BC.CASES[BC.IDS.index(f"sweep_d{d}")])
        S, windows = _windowed_sums(X, Y, ks, BC.kw_max(d))
        assert len(windows) == 2 and not np.isnan(S).any()
        (_, _, m0a, mla), (c0b, _, m0b, _) = windows
        assert m0b == m0a + mla - 1 == 9 and BC.offsets(ks)[9] < c0b < BC.offsets(ks)[10]     # k = 11 straddles
        off = BC.offsets(ks)
        for m in range(len(ks)):
            assert S[:, off[m]:off[m + 1]].tobytes() == MT.silhouette_sums_f32(X, Y[m]).tobytes(), (d, m)
