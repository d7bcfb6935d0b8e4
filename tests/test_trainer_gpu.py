"""The fused Trainer step (one native call sequence, no host sync) equals the autograd path
(model -> loss_function -> backward -> hlmc Adam) bit-for-bit up to float rounding."""
import pytest
import torch

import hlmc_amd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("audio_only", [False, True])
def test_trainer_equals_autograd_path(cuda, audio_only):
    torch.manual_seed(42)
    a = hlmc_amd.HybridVAE(128, 384, (128, 128), audio_only=audio_only).cuda()
    torch.manual_seed(42)
    b = hlmc_amd.HybridVAE(128, 384, (128, 128), audio_only=audio_only).cuda()
    opt = hlmc_amd.Adam(a.parameters(), lr=1e-4)
    tr = hlmc_amd.Trainer(b, lr=1e-4)
    g = torch.Generator().manual_seed(0)
    for step in range(3):
        audio = torch.randn(8, 1, 128, 128, generator=g).cuda()
        text = (torch.randn(8, 384, generator=g) / 384 ** 0.5).cuda()
        eps = torch.randn(8, 128, generator=g).cuda()
        opt.zero_grad()
        out = a(audio, None if audio_only else text, eps=eps)
        loss = hlmc_amd.loss_function(out[0], audio, out[1], None if audio_only else text, out[2], out[3])
        loss[0].backward()
        opt.step()
        sums = tr.step(audio, None if audio_only else text, eps=eps)
        tot = tr.loss_tuple(sums)[0]
        assert abs(tot - float(loss[0])) <= 1e-6 * abs(float(loss[0]))
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7, msg=n)


def test_trainer_bf16_loss_decreases(cuda):
    torch.manual_seed(0)
    m = hlmc_amd.HybridVAE(128, 384, (128, 128), audio_only=True, compute_dtype="bf16").cuda()
    tr = hlmc_amd.Trainer(m, lr=1e-3)
    g = torch.Generator(device=cuda).manual_seed(1)
    audio = torch.randn(32, 1, 128, 128, device=cuda, generator=g)
    first = last = None
    for i in range(20):
        tot = tr.loss_tuple(tr.step(audio))[0]
        first = tot if first is None else first
        last = tot
    assert last < 0.9 * first


@pytest.mark.parametrize("kind", ["hybrid", "cvae"])
def test_trainer_dp_overlapped_allreduce_world1(cuda, kind):
    """The DP path (per-bucket RCCL all-reduces on a comm stream gated on backward's bucket events, Adam
    waiting on them) in a 1-rank NCCL group: parameters must equal the non-distributed Trainer's exactly."""
    import os
    import torch.distributed as dist
    own = not dist.is_initialized()
    if own:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 1000))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=cuda)
    try:
        def make():
            torch.manual_seed(42)
            if kind == "hybrid":
                m = hlmc_amd.HybridVAE(128, 384, (128, 128), compute_dtype="bf16").cuda()
            else:
                m = hlmc_amd.ConditionalVAE(64, 384, 10, (128, 128), compute_dtype="bf16").cuda()
            return m
        a, b = make(), make()
        ta = hlmc_amd.Trainer(a, lr=1e-3)
        tb = hlmc_amd.Trainer(b, lr=1e-3, distributed=True)
        assert len(tb.buckets) >= 3
        g = torch.Generator().manual_seed(0)
        for _ in range(3):
            audio = torch.randn(16, 1, 128, 128, generator=g).cuda()
            text = (torch.randn(16, 384, generator=g) / 384 ** 0.5).cuda()
            eps = torch.randn(16, a.latent_dim, generator=g).cuda()
            extra = ()
            if kind == "cvae":
                extra = (torch.nn.functional.one_hot(torch.arange(16) % 10, 10).float().cuda(),)
            sa = ta.step(audio, text, *extra, eps=eps)
            sb = tb.step(audio, text, *extra, eps=eps)
            assert torch.equal(sa, sb)
        torch.cuda.synchronize()
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), n
    finally:
        if own:
            dist.destroy_process_group()


def test_graphed_step_equals_eager(cuda):
    """GraphedStep (whole step captured into a HIP graph, Adam coefficients staged per replay) updates the
    parameters exactly like eager Trainer.step on the same batches."""
    def make():
        torch.manual_seed(42)
        return hlmc_amd.HybridVAE(128, 384, (128, 128), compute_dtype="bf16").cuda()
    a, b = make(), make()
    ta = hlmc_amd.Trainer(a, lr=1e-3)
    tb = hlmc_amd.Trainer(b, lr=1e-3)
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(8, 1, 128, 128, generator=g), torch.randn(8, 384, generator=g) / 384 ** 0.5,
                torch.randn(8, 128, generator=g)) for _ in range(4)]
    audio, text, eps = (t.clone().cuda() for t in batches[0])

    def body():
        return tb.step(audio, text, eps=eps)

    gs = hlmc_amd.GraphedStep(tb, body, warmup=1)   # the warmup is batch 0's real step
    for i, (x, t, e) in enumerate(batches):
        sa = ta.step(x.cuda(), t.cuda(), eps=e.cuda())
        if i > 0:
            audio.copy_(x)
            text.copy_(t)
            eps.copy_(e)
            sb = gs()
            torch.cuda.synchronize()
            assert torch.equal(sa, sb), i
    torch.cuda.synchronize()
    assert ta.step_count == tb.step_count == 4
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    gs.release()


def test_checkpoint_resume_restores_noise_stream(cuda):
    """model.state_dict() + Trainer.state_dict() (Adam moments, step count, the engine's Philox (seed, offset))
    resume a run bit for bit, device-drawn reparameterisation noise included."""
    def make():
        torch.manual_seed(42)
        m = hlmc_amd.HybridVAE(128, 384, (128, 128), audio_only=True).cuda()
        return m, hlmc_amd.Trainer(m, lr=1e-3)

    g = torch.Generator().manual_seed(3)
    batches = [torch.randn(8, 1, 128, 128, generator=g).cuda() for _ in range(3)]
    m, tr = make()
    for x in batches[:2]:
        tr.step(x)
    ck_model = {k: v.clone() for k, v in m.state_dict().items()}
    ck_tr = tr.state_dict()
    assert ck_tr["rng"][1] > 0   # the offset advanced past the two steps' draws
    tr.step(batches[2])
    want = {k: v.clone() for k, v in m.state_dict().items()}
    m2, tr2 = make()
    m2.load_state_dict(ck_model)
    tr2.load_state_dict(ck_tr)
    tr2.step(batches[2])
    for k, v in m2.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_rng_state_round_trip(cuda):
    torch.manual_seed(7)
    m = hlmc_amd.HybridVAE(128, 384, (128, 128), audio_only=True).cuda()
    st = m.get_rng_state()
    assert st[0] == 7
    m.set_rng_state((123, 456))
    assert m.get_rng_state() == (123, 456)


# ------------------------------------------------------------------ the fused Adam + weight-pack step, op level
ADAM_HP = dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-2)
KINDS = ["hybrid", "cvae", "simple"]


def _make(kind, dtype, seed=42):
    torch.manual_seed(seed)
    if kind == "hybrid":
        return hlmc_amd.HybridVAE(128, 384, (128, 128), compute_dtype=dtype).cuda()
    if kind == "cvae":
        return hlmc_amd.ConditionalVAE(64, 384, 10, (128, 128), compute_dtype=dtype).cuda()
    return hlmc_amd.VAE(370, [128, 64, 32], 32, compute_dtype=dtype).cuda()


def _batches(kind, model, B, steps, seed=0):
    """Per step: (positional inputs of Trainer.step / the model's forward, eps, dropout keep-mask or None)."""
    g = torch.Generator().manual_seed(seed)
    gd = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for _ in range(steps):
        eps = torch.randn(B, model.latent_dim, generator=g).cuda()
        if kind == "simple":
            x = torch.randn(B, 370, generator=g).cuda()
            out.append(((x,), eps, model.make_dropout_mask(B, x.device, generator=gd)))
            continue
        ins = (torch.randn(B, 1, 128, 128, generator=g).cuda(), (torch.randn(B, 384, generator=g) / 384 ** 0.5).cuda())
        if kind == "cvae":
            ins += (torch.nn.functional.one_hot(torch.arange(B) % 10, 10).float().cuda(),)
        out.append((ins, eps, None))
    return out


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().numpy()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_adam_matches_float64(cuda, kind, dtype):
    """adam_pack_kernel's arithmetic, isolated from the model: over 3 Trainer steps with non-default
    hyper-parameters and weight decay, every new parameter and both moments against oracle/optim_oracle.adam_step
    applied to the step's own inputs (parameters and moments cloned before it, the gradient it left in gflat).
    Covers the float4 and the per-element path, tiles ragged in both directions (370 = 5 * 64 + 50, the CVAE's
    74-wide decoder input), the unpacked 4096-element chunks and both pack types.

    Bounds: tests.test_optim_gpu.adam_bounds(cancelling=True) -- model gradients may cancel against wd * p.  The
    float32 restatement of the kernel (adam_fp32) is checked against the same bounds on the same tensors first;
    the share of elements at which it leaves them must be 0.

    Measured on MI355X, worst |err| / bound over the six cases: p 0.63, m 0.25, v 0.60; restatement outside: 0."""
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from tests.test_optim_gpu import adam_bounds, adam_fp32, f32_hyper, worst_ratio

    model = _make(kind, dtype)
    tr = hlmc_amd.Trainer(model, **ADAM_HP)
    hp = f32_hyper(ADAM_HP["lr"], ADAM_HP["betas"], ADAM_HP["eps"], ADAM_HP["weight_decay"])
    params = list(model.parameters())
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    outside = 0
    for step, (ins, eps, mask) in enumerate(_batches(kind, model, 4, 3), start=1):
        before = (_flat(params), tr.m.cpu().numpy(), tr.v.cpu().numpy())
        tr.step(*ins, eps=eps, dropout=mask)
        torch.cuda.synchronize()
        grad = tr.gflat.cpu().numpy()
        after = (_flat(params), tr.m.cpu().numpy(), tr.v.cpu().numpy())
        assert tr.step_count == step and np.all(np.isfinite(grad)) and np.any(grad != 0)

        def chunk(lo):
            sl = slice(lo, lo + (1 << 20))
            args = (before[0][sl], grad[sl], before[1][sl], before[2][sl])
            ref, bnd = adam_bounds(*args, *hp, step, cancelling=True)
            cpu = adam_fp32(*args, *hp, step)
            bad = sum(int(np.count_nonzero(np.abs(c.astype(np.float64) - r) > b)) for c, r, b in zip(cpu, ref, bnd))
            return bad, [worst_ratio(a[sl], r, b) for a, r, b in zip(after, ref, bnd)]

        with ThreadPoolExecutor(8) as pool:
            for bad, rs in pool.map(chunk, range(0, grad.size, 1 << 20)):
                outside += bad
                for k, r in zip("pmv", rs):
                    worst[k] = max(worst[k], r)
    n = 3 * 3 * tr.gflat.numel()
    print(f"{kind} {dtype}: fused Adam worst |err| / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}; "
          f"float32 restatement outside its bound at {outside} of {n} values")
    assert outside == 0, "the bound does not hold for the reference arithmetic itself"
    assert max(worst.values()) <= 1.0, worst
    tr.release()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_adam_written_packs_equal_fresh_packs(cuda, kind, dtype):
    """The packed GEMM weights adam_pack_kernel wrote (P0 / P1, trusted by the Trainer's net) against pack_kernel's
    fresh packs of the same weights: after 3 steps, the trained model's eval-mode outputs equal, bit for bit, those
    of a new model that loaded its state_dict (whose forward re-packs).  The weights themselves are compared with
    the float64 reference in test_fused_adam_matches_float64."""
    model = _make(kind, dtype)
    tr = hlmc_amd.Trainer(model, **ADAM_HP)
    for ins, eps, mask in _batches(kind, model, 4, 3):
        tr.step(*ins, eps=eps, dropout=mask)
    model.eval()
    fresh = _make(kind, dtype, seed=1)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    (ins, eps, _), = _batches(kind, model, 4, 1, seed=5)
    with torch.no_grad():
        got, want = model(*ins, eps=eps), fresh(*ins, eps=eps)   # the trained net still trusts its own packs
        if kind == "hybrid":
            got, want = got + model.encode(*ins), want + fresh.encode(*ins)
    torch.cuda.synchronize()
    assert len(got) == len(want) >= 4
    for k, (x, y) in enumerate(zip(got, want)):
        assert torch.isfinite(x).all() and torch.equal(x, y), k
    # not vacuous: the trained net really reads the packs Adam wrote, not the weights (a weight changed behind its
    # back, as hlmc.h forbids under trust, goes unseen)
    w = max(model.parameters(), key=lambda p: p.numel())
    with torch.no_grad():
        w.mul_(2.0)
        again = model(*ins, eps=eps)
        w.mul_(0.5)
    assert torch.equal(again[0], got[0])
    tr.release()


def test_simple_vae_trainer_equals_autograd_path(cuda):
    """Trainer on the Simple VAE (mean-mode loss coefficients, dropout masks, 370-wide weights ragged in both tile
    directions) equals model -> vae_loss(beta=0.8) -> backward -> hlmc Adam on the same masks and eps."""
    a, b = _make("simple", "fp32"), _make("simple", "fp32")
    opt = hlmc_amd.Adam(a.parameters(), lr=1e-4)
    tr = hlmc_amd.Trainer(b, lr=1e-4)
    assert tr.kind == "simple" and tr.beta == 0.8
    for (x,), eps, mask in _batches("simple", a, 8, 3):
        opt.zero_grad()
        out = a(x, eps=eps, dropout_mask=mask)
        loss = hlmc_amd.vae_loss(out[0], x, out[1], out[2], beta=0.8)
        loss[0].backward()
        opt.step()
        tot = tr.loss_tuple(tr.step(x, eps=eps, dropout=mask))[0]
        want = float(loss[0].detach())
        assert abs(tot - want) <= 1e-6 * abs(want)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7, msg=n)
    for (n, p), q in zip(a.named_buffers(), b.buffers()):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7, msg=n)
    tr.release()


def test_overlap_adam_equals_default(cuda, monkeypatch):
    """HLMC_OVERLAP_ADAM=1 (the Adam step as two launches split at the late parameters, the first under the tail of
    the backward pass) leaves the same sums, parameters and moments as the default single launch, bit for bit.
    The engine has no query for whether the split path ran (it also needs its side stream, no bucket sync and late
    parameters, all true for this single-process Hybrid model): were the variable ignored, this would pass too."""
    monkeypatch.delenv("HLMC_OVERLAP_ADAM", raising=False)
    a, b = _make("hybrid", "bf16"), _make("hybrid", "bf16")
    ta = hlmc_amd.Trainer(a, lr=1e-3)
    monkeypatch.setenv("HLMC_OVERLAP_ADAM", "1")
    tb = hlmc_amd.Trainer(b, lr=1e-3)
    for ins, eps, _ in _batches("hybrid", a, 8, 3):
        sa = ta.step(*ins, eps=eps).clone()
        sb = tb.step(*ins, eps=eps).clone()
        assert torch.equal(sa, sb)
    torch.cuda.synchronize()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    assert torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    assert float(ta.v.sum()) > 0
    ta.release()
    tb.release()
