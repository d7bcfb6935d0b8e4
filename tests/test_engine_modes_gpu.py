"""Engine schedule modes that no other test reaches.

  * single-stream mode (``HLMC_SIDE_STREAM=0``): every weight and bias gradient on the caller's
    stream.  The variable is read once per process, so the check runs in a fresh child process; there the model
    step is compared with the oracle by ``test_models_gpu.compare_step`` at its usual tolerances.
  * ``hlmc_net_backward`` twice after one ``hlmc_net_forward``: the second call has to clear the BatchNorm-backward
    accumulators itself (the forward's memset covered only the first), so it must reproduce the first bit for bit.
"""
import os
import subprocess
import sys

import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE_STREAM_CASES = ["audio_128x128", "cvae_128x128", "simple_370"]


def single_stream_child():
    """Runs in the child process of test_single_stream_mode_matches_oracle."""
    from tests import test_models_gpu as TM
    from tests.golden import fixtures as FX

    assert os.environ.get("HLMC_SIDE_STREAM") == "0"
    for name in SINGLE_STREAM_CASES:
        case = FX.case_by_name(name)
        ora, ours = TM.build(case)
        TM.compare_step(case, ora, ours)
        print(f"single-stream {name}: ok", flush=True)


def test_single_stream_mode_matches_oracle(cuda):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_engine_modes_gpu import single_stream_child; " \
           "single_stream_child()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, env=dict(os.environ, HLMC_SIDE_STREAM="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    for name in SINGLE_STREAM_CASES:
        assert f"single-stream {name}: ok" in r.stdout


def test_backward_twice_after_one_forward(cuda):
    B, latent, H = 2, 8, 64
    torch.manual_seed(42)
    ours = hlmc_amd.HybridVAE(latent_dim=latent, text_dim=768, input_hw=(H, H), audio_only=True).cuda().train()
    net = ours._native_net()
    g = torch.Generator().manual_seed(11)
    audio = torch.randn(B, 1, H, H, generator=g).cuda()
    eps = torch.randn(B, latent, generator=g).cuda()
    d_recon = torch.randn(B, 1, H, H, generator=g).cuda()
    d_mu = torch.randn(B, latent, generator=g).cuda()
    d_lv = torch.randn(B, latent, generator=g).cuda()
    recon = torch.empty(B, 1, H, H, device="cuda")
    mu = torch.empty(B, latent, device="cuda")
    lv = torch.empty(B, latent, device="cuda")
    ws = net.new_workspace(B, audio.device)
    lib = L.lib()
    L.check(lib.hlmc_net_forward(net.h, L.stream(), B, 1, L.ptr(audio), None, None, L.ptr(eps), None, L.ptr(recon), None,
                                 L.ptr(mu), L.ptr(lv), None, ws.data_ptr()), "hlmc_net_forward")
    grads = []
    for _ in range(2):
        ours._gflat.zero_()
        L.check(lib.hlmc_net_backward(net.h, L.stream(), B, L.ptr(d_recon), None, L.ptr(d_mu), L.ptr(d_lv),
                                      ws.data_ptr()), "hlmc_net_backward")
        L.check(lib.hlmc_net_settle(net.h, L.stream()), "hlmc_net_settle")
        torch.cuda.synchronize()
        grads.append(ours._gflat.clone())
    assert torch.isfinite(grads[0]).all() and float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1]), f"max |first - second| = {float((grads[0] - grads[1]).abs().max()):.3e}"
