"""The dense middle without its relayout / reparameterisation launches and with the latent heads as one GEMM per
direction, against oracle/models_oracle.py on the same state_dict, input and eps.

What can go wrong, and the smallest shapes that show it:
  * the NHWC <-> NCHW-flat permutation now rides in the stores of four producers (the encoder's last BatchNorm pass,
    audio_decoder_fc's and audio_fc's data-gradient epilogues, the first decoder layer's data gradient).  At 64 x 128
    and 128 x 64 the low-res map has hw = 2 pixels with h != w, so a transposed or inverted permutation gives O(1)
    errors in audio_fc.weight, audio_decoder_fc.weight / .bias and every encoder gradient; 128 x 128 is the bench shape
    (hw = 4).  B = 5 is odd: no multiple of a tile, of the 4-wide Philox groups or of a float4.
  * fc_mu / fc_logvar share one packed weight and one weight-gradient launch whose epilogue splits the rows.
  * the reparameterisation runs inside the heads' reduce launch (forward) and inside the reduce of
    decoder_input's data gradient (backward).

Tolerances are test_models_gpu.py's (imported, not restated): outputs / losses 1e-4, per-parameter gradients within
max(1e-3, 8 x the fp32 oracle's own error vs float64) plus the kink envelope, BN-fed biases absolutely, bf16 under
test_bf16_mode_tracks_fp32's rules."""
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import models_oracle as OM
from tests import test_models_gpu as TM

pytestmark = pytest.mark.gpu

rel = TM.rel


def _case(kind, hw, B, audio_only=False, **ctor):
    return dict(name=f"{kind}_{hw[0]}x{hw[1]}_b{B}", kind=kind, hw=hw, B=B, audio_only=audio_only, ctor=ctor)


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("hw", [(64, 128), (128, 64), (128, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_layout_fold_fp32(cuda, hw, B):
    """Audio-only HybridVAE, one train-mode forward + backward: recon, mu, logvar, the loss and every parameter
    gradient (and the BatchNorm buffers) at the fp32 contract."""
    case = _case("hybrid", hw, B, audio_only=True, latent_dim=128, text_dim=768)
    ora, ours = TM.build(case)
    TM.compare_step(case, ora, ours)


def test_layout_fold_bf16(cuda):
    """64 x 128, B = 5 in the throughput mode, under test_bf16_mode_tracks_fp32's rules."""
    case = _case("hybrid", (64, 128), 5, audio_only=True, latent_dim=128, text_dim=768)
    ora, ours = TM.build(case, "bf16")
    ins, eps = TM.FX.inputs_fn(case)(0)
    o_out, o_loss = TM.run_oracle_step(case, ora, ins, eps)
    m_out, m_loss = TM.run_ours_step(case, ours, ins, eps)
    e_mu = rel(m_out[2].detach(), o_out[2].detach())
    e_loss = abs(float(m_loss[0]) - float(o_loss[0])) / abs(float(o_loss[0]))
    gm = torch.cat([p.grad.reshape(-1).cpu() for p in ours.parameters()])
    go = torch.cat([p.grad.reshape(-1) for p in ora.parameters()])
    errs = {n: rel(p.grad, q.grad) for (n, p), q in zip(ours.named_parameters(), ora.parameters())
            if not TM._bias_feeds_bn(ora, n)}
    print(f"bf16 64x128 B=5: mu {e_mu:.2e} loss {e_loss:.2e} grad {rel(gm, go):.2e}; worst",
          sorted(errs.items(), key=lambda kv: -kv[1])[:6])
    assert e_mu < 3e-2
    assert e_loss < 2e-2
    # (a wrong permutation is O(1) in audio_fc.weight, audio_decoder_fc.weight and every encoder gradient, i.e. in
    # most of the gradient's norm: far outside the overall bound; the per-tensor figures are printed above)
    assert rel(gm, go) < 0.15
    bo = dict(ora.named_buffers())
    for n, b in ours.named_buffers():
        if b.dtype.is_floating_point:
            assert rel(b.detach(), bo[n]) < 5e-2, n
        else:
            assert torch.equal(b.detach().cpu(), bo[n]), n


@pytest.mark.parametrize("case", [
    _case("hybrid", (64, 128), 5, latent_dim=128, text_dim=384),
    _case("cvae", (64, 64), 5, latent_dim=64, text_dim=768, num_classes=10),
    _case("cvae", (64, 128), 5, latent_dim=64, text_dim=768, num_classes=10),
], ids=lambda c: c["name"])
def test_other_models_fp32(cuda, case):
    """HybridVAE with its text branch, and the ConditionalVAE (its smallest shape, and the smallest with hw > 1):
    the CVAE's decoder_fc / head data gradients write part of their columns in NHWC order and the rest row-major."""
    ora, ours = TM.build(case)
    TM.compare_step(case, ora, ours)


@pytest.mark.parametrize("latent_grads", [True, False], ids=["with_dmu_dlv", "without"])
def test_merged_heads_gradients(cuda, latent_grads):
    """fc_mu / fc_logvar weight and bias gradients, each on its own, after one step at B = 5: with the caller's
    d_mu / d_logvar (what the Trainer's KL term supplies) and with a loss that does not read mu / logvar (autograd
    passes no gradient for them; the engine sees zeros).  Bound per tensor: relative
    L2 error vs a float64 oracle run <= max(1e-3, 8 x the fp32 oracle's own error) (test_models_gpu.py's rule without
    its kink allowance)."""
    B, hw = 5, (64, 128)
    ctor = dict(latent_dim=128, text_dim=768, input_hw=hw, audio_only=True)
    torch.manual_seed(42)
    ora = OM.HybridVAE(**ctor).train()
    torch.manual_seed(42)
    ours = hlmc_amd.HybridVAE(**ctor).cuda()
    g = torch.Generator().manual_seed(11)
    audio = torch.randn(B, 1, *hw, generator=g)
    eps = torch.randn(B, 128, generator=g)
    d_recon = torch.randn(B, 1, *hw, generator=g) / 64
    d_mu = torch.randn(B, 128, generator=g) if latent_grads else None
    d_lv = torch.randn(B, 128, generator=g) if latent_grads else None

    def oracle_grads(model, dt):
        model.zero_grad()
        o = model(audio.to(dt), None, eps=eps.to(dt))
        loss = (o[0] * d_recon.to(dt)).sum()
        if latent_grads:
            loss = loss + (o[2] * d_mu.to(dt)).sum() + (o[3] * d_lv.to(dt)).sum()
        loss.backward()
        return o, {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    import copy
    _, g64 = oracle_grads(copy.deepcopy(ora).double(), torch.float64)
    o32, g32 = oracle_grads(ora, torch.float32)
    ours.train()
    m = ours(audio.cuda(), None, eps=eps.cuda())
    loss = (m[0] * d_recon.cuda()).sum()
    if latent_grads:
        loss = loss + (m[2] * d_mu.cuda()).sum() + (m[3] * d_lv.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    gm = {n: p.grad.detach().cpu() for n, p in ours.named_parameters()}
    for k in (0, 2, 3):  # recon, mu, logvar
        assert rel(m[k].detach(), o32[k].detach()) < 1e-4, k
    for n in ("fc_mu.weight", "fc_mu.bias", "fc_logvar.weight", "fc_logvar.bias", "fc_fusion.weight",
              "decoder_input.weight"):
        e_ref, e_ours = rel(g32[n], g64[n]), rel(gm[n], g64[n])
        print(f"{n}: engine {e_ours:.2e}, fp32 oracle {e_ref:.2e}")
        assert e_ours <= max(1e-3, 8 * e_ref), f"{n}: {e_ours:.3e} vs fp32 oracle {e_ref:.3e}"


def test_device_noise_stream_and_offsets(cuda):
    """eps = None: two consecutive train-mode forwards draw from the net's Philox stream inside the heads' reduce
    launch.  They must equal, bit for bit, the same forwards fed the eps hlmc_randn returns for the same seed at
    offsets 0 and round-up-to-4(B * L): this pins the stream elements and the offset bookkeeping.  B * L = 630 is no
    multiple of 4 (the last Philox group is partial and the next forward starts at 632)."""
    B, Ld, hw, seed = 5, 126, (64, 128), 1234
    ctor = dict(latent_dim=Ld, text_dim=768, input_hw=hw, audio_only=True)

    def fresh():
        torch.manual_seed(42)
        m = hlmc_amd.HybridVAE(**ctor).cuda().train()
        m.set_rng_state((seed, 0))
        return m

    g = torch.Generator().manual_seed(3)
    audios = [torch.randn(B, 1, *hw, generator=g).cuda() for _ in range(2)]
    a, b = fresh(), fresh()
    step = (B * Ld + 3) // 4 * 4
    with torch.no_grad():
        got, want = [], []
        for i, audio in enumerate(audios):
            got.append(a(audio, None))
            eps = torch.empty(B, Ld, device="cuda")
            L.check(L.lib().hlmc_randn(L.stream(), eps.data_ptr(), eps.numel(), seed, i * step))
            want.append(b(audio, None, eps=eps))
    torch.cuda.synchronize()
    assert a.get_rng_state() == (seed, 2 * step)
    assert b.get_rng_state() == (seed, 0)
    for x, y in zip(got, want):
        for k in (0, 2, 3):  # recon, mu, logvar
            assert torch.isfinite(x[k]).all() and torch.equal(x[k], y[k]), k
    assert not torch.equal(got[0][0], got[1][0])


def test_eval_encode_decode(cuda):
    """Eval-mode forward, encode and decode at 64 x 128, B = 3 (the paths that share the new stores)."""
    case = _case("hybrid", (64, 128), 3, latent_dim=128, text_dim=384)
    ora, ours = TM.build(case)
    ins, eps = TM.FX.inputs_fn(case)(0)
    cins = [t.cuda() for t in ins]
    ora.eval()
    ours.eval()
    z = torch.randn(3, 128, generator=torch.Generator().manual_seed(77))
    with torch.no_grad():
        o_out = ora(*ins, eps=eps)
        m_out = ours(*cins, eps=eps.cuda())
        mo, lo = ora.encode(*ins)
        mm, lm = ours.encode(*cins)
        ro = ora.decode(z)
        rm = ours.decode(z.cuda())
    for i, (x, y) in enumerate(zip(m_out, o_out)):
        assert rel(x, y) < 1e-4, f"eval output {i}: {rel(x, y):.2e}"
    assert rel(mm, mo) < 1e-5 and rel(lm, lo) < 1e-5
    for x, y in zip(rm, ro):
        assert rel(x, y) < 1e-4
    for (n, bo), (_, bm) in zip(ora.named_buffers(), ours.named_buffers()):
        assert torch.equal(bm.cpu(), bo), n
