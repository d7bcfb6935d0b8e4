"""SimpleAutoencoder baseline (src/Conditional_VAE.py:252-273 and its loop at :428-452), the parts that need no GPU:
the engine's kind 3 layout, the host-side argument checks of the two new entry points, the DataLoader row order, the
module's state dict, and the numpy restatement of hlmc_mse_rows that the GPU test shares (tests/ae_check.py)."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import models_oracle as OM
from tests import ae_check as AE

ONE = C.c_void_p(256)          # non-null placeholder: validation fails before anything is dereferenced
NULL = None


def _create(cfg, kind=3, dtype=0):
    h = C.c_void_p()
    st = L.lib().hlmc_net_create(kind, L.i64_array(cfg), len(cfg), dtype, C.byref(h))
    return st, h


def _err():
    return L.lib().hlmc_last_error().decode()


@pytest.mark.parametrize("dtype", [L.HLMC_F32, L.HLMC_BF16])
def test_kind3_layout_is_the_oracles(dtype):
    st, h = _create([290, 64], dtype=dtype)
    assert st == 0, _err()
    lib = L.lib()
    want = [(n, tuple(p.shape)) for n, p in OM.SimpleAutoencoder(290, 64).named_parameters()]
    assert lib.hlmc_net_num_params(h) == len(want) == 12
    got = []
    for i in range(len(want)):
        name, nd, shape = C.create_string_buffer(256), C.c_int(), (C.c_int64 * 4)()
        assert lib.hlmc_net_param_info(h, i, name, 256, C.byref(nd), shape) == 0
        got.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
    assert got == want
    assert lib.hlmc_net_num_bn(h) == 0
    assert lib.hlmc_net_state_bytes(h) > 0 and lib.hlmc_net_workspace_bytes(h, 1) > 0
    assert lib.hlmc_net_workspace_bytes(h, 33) >= lib.hlmc_net_workspace_bytes(h, 32)
    lib.hlmc_net_destroy(h)


@pytest.mark.parametrize("cfg", [[290], [290, 64, 1], [0, 64], [290, 0], [-3, 64], [290, -1]])
def test_kind3_bad_cfg_is_refused_with_a_message(cfg):
    st, _ = _create(cfg)
    assert st == -1 and "autoencoder" in _err()


def test_odd_dims_are_accepted_and_kind7_stays_invalid():
    for cfg in ([1, 1], [13, 6], [8, 64]):
        st, h = _create(cfg)
        assert st == 0, _err()
        L.lib().hlmc_net_destroy(h)
    st, _ = _create([290, 64], kind=7)
    assert st == -1 and "unknown net kind" in _err()


GATHER_OK = dict(X=ONE, n=10, d=4, idx=ONE, count=3, B=4, out=ONE, valid=ONE)


@pytest.mark.parametrize("bad", [dict(X=NULL), dict(idx=NULL), dict(out=NULL), dict(valid=NULL), dict(count=0),
                                 dict(count=5), dict(count=-1), dict(d=0), dict(d=-4), dict(n=0), dict(B=0)])
def test_batch_gather_checks_its_arguments_on_the_host(bad):
    a = {**GATHER_OK, **bad}
    st = L.lib().hlmc_batch_gather(None, a["X"], a["n"], a["d"], a["idx"], a["count"], a["B"], a["out"], a["valid"])
    assert st == -1 and "batch_gather" in _err()


MSE_OK = dict(recon=ONE, target=ONE, B=4, d=3, valid=ONE, d_recon=ONE, sums2=ONE, acc=ONE, ws=ONE)


@pytest.mark.parametrize("bad", [dict(recon=NULL), dict(target=NULL), dict(valid=NULL), dict(d_recon=NULL),
                                 dict(sums2=NULL), dict(ws=NULL), dict(d=0), dict(d=-1), dict(B=0)])
def test_mse_rows_checks_its_arguments_on_the_host(bad):
    a = {**MSE_OK, **bad}
    st = L.lib().hlmc_mse_rows(None, a["recon"], a["target"], a["B"], a["d"], a["valid"], a["d_recon"], a["sums2"],
                               a["acc"], a["ws"])
    assert st == -1 and "mse_rows" in _err()


def test_mse_rows_workspace_is_monotone():
    f = L.lib().hlmc_mse_rows_workspace
    sizes = [1, 2, 13, 32, 33, 256, 290, 1024, 4096, 100000]
    for d in sizes:
        col = [f(B, d) for B in sizes]
        assert col[0] >= 8 and all(a <= b for a, b in zip(col, col[1:])), (d, col)
    for B in sizes:
        row = [f(B, d) for d in sizes]
        assert all(a <= b for a, b in zip(row, row[1:])), (B, row)
    assert f(0, 4) == 0 and f(4, 0) == 0 and f(-1, 4) == 0
    assert f(256, 4096) > f(32, 290)   # the two-launch form needs room for its block totals


@pytest.mark.parametrize("n", [1, 33, 77])
@pytest.mark.parametrize("explicit", [False, True])
def test_dataloader_order_is_the_live_dataloaders(n, explicit):
    """Three consecutive epochs of DataLoader(shuffle=True) at batch 32, against dataloader_order cut into batches, from
    the same generator state; afterwards both generators are in the same state."""
    data = torch.arange(n)

    def gens():
        torch.manual_seed(1234 + n)
        return torch.Generator().manual_seed(99 + n) if explicit else None

    g = gens()
    loader = DataLoader(TensorDataset(data), batch_size=32, shuffle=True, generator=g)
    want = [[b[0].tolist() for b in loader] for _ in range(3)]
    state_want = (g.get_state() if explicit else torch.get_rng_state()).clone()
    g = gens()
    got = []
    for _ in range(3):
        order = hlmc_amd.dataloader_order(n, g)
        assert order.dtype == torch.int64 and sorted(order.tolist()) == list(range(n))
        got.append([order[k:k + 32].tolist() for k in range(0, n, 32)])
    assert got == want
    assert torch.equal(g.get_state() if explicit else torch.get_rng_state(), state_want)


@pytest.mark.parametrize("B,d,valid", AE.MSE_CASES)
def test_numpy_restatement_of_mse_rows_is_inside_its_bounds(B, d, valid):
    """tests/ae_check.py mse_rows_f32 (float32 inputs, the kernel's float64 arithmetic in numpy's pairwise order)
    against the exact values (Fraction-free: math.fsum of exactly representable products where it matters) at the
    bounds the GPU test applies to the kernel."""
    recon, target = AE.mse_inputs(B, d)
    g, sums = AE.mse_rows_f32(recon, target, valid)
    AE.check_mse(recon, target, valid, g, sums)


def test_state_dict_equals_the_oracles_under_the_same_seed():
    torch.manual_seed(42)
    ora = OM.SimpleAutoencoder(290, 64)
    torch.manual_seed(42)
    ours = hlmc_amd.SimpleAutoencoder(290, 64)
    so, sm = ora.state_dict(), ours.state_dict()
    assert list(so) == list(sm)
    for k in so:
        assert torch.equal(so[k], sm[k]), k
    ora.load_state_dict(sm)   # interchangeable files


def test_module_refuses_the_cpu():
    m = hlmc_amd.SimpleAutoencoder(13, 6)
    x = torch.zeros(4, 13)
    with pytest.raises(L.HLMCError, match="GPU tensors"):
        m(x)
    with pytest.raises(L.HLMCError):
        m.encode(x)
    with pytest.raises(L.HLMCError):
        hlmc_amd.fit_autoencoder(m, x, epochs=1)
    with pytest.raises(ValueError):
        hlmc_amd.SimpleAutoencoder(13, 6, compute_dtype="fp16")


def test_new_symbols_are_bound_and_exported():
    for s in ("hlmc_batch_gather", "hlmc_mse_rows", "hlmc_mse_rows_workspace"):
        assert s in L.exported_symbols() and hasattr(L.lib(), s)
    for s in ("SimpleAutoencoder", "AutoencoderTrainer", "fit_autoencoder", "dataloader_order",
              "autoencoder_kmeans_baseline", "direct_kmeans_baseline"):
        assert s in hlmc_amd.__all__ and hasattr(hlmc_amd, s)
