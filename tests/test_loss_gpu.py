"""The loss kernels (hlmc_loss_sums, hlmc_loss_backward, hlmc_loss_sums_backward) and their autograd wrapper
(loss_function, cvae_loss_function, vae_loss) against float64 references.

The C entry points are compared with oracle/optim_oracle.loss_sums_and_grads (numpy float64 on the float32 inputs),
the wrappers with oracle/models_oracle's loss functions under torch float64 autograd, for several scalars of the
returned tuple so that every upstream gradient (total, audio, text, kld) and the mean-mode scaling take part.
All bounds count roundings, u = 2^-24:

    sums[0], sums[1]   4u relative (one float32 rounding of the difference, double squares and sums)
    sums[2]            8u sum(1 + |lv| + mu^2 + e^lv)
    d ra, d rt         4u |ref|      d mu   2u |ref|      d lv   4u |ck| (1 + e^lv)

Measured on MI355X, worst |err| / bound: kernels -- sums 0.30 / 0.20 / 0.09, d ra 0.25, d rt 0.41, d lv 0.14 (d mu
exact: ck = 4); wrappers -- d ra 0.48, d rt 0.36, d mu 0.70, d lv 0.20.
"""
import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import models_oracle as OM
from oracle import optim_oracle as OO

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
COEF = (2.0, 700.0, 4.0)
SENT, SPARE = -12345.5, 8


def grad_bounds(ref_dra, ref_drt, ref_dmu, lv, ck):
    return (4 * U * np.abs(ref_dra), None if ref_drt is None else 4 * U * np.abs(ref_drt), 2 * U * np.abs(ref_dmu),
            4 * U * abs(ck) * (1.0 + np.exp(np.asarray(lv, dtype=np.float64))))


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("na,nt,nl", [(1, 0, 1), (255, 1, 3), (2049, 383, 130), (130, 0, 2049),
                                      (4 * 128 * 128 + 3, 4 * 384, 4 * 128), (2048 * 1024 + 5, 0, 7)])
def test_loss_kernels_match_float64(cuda, na, nt, nl):
    """The three entry points at ragged sizes, nl > na (the latent count sizes the grid), a size past the
    1024-block grid cap (the grid-stride loops iterate twice), logvar in [-12, 6]; fused == separate bit for bit;
    nothing written past the outputs' ends."""
    rng = np.random.default_rng(na + 7 * nt + 13 * nl)

    def f32(x):
        return x.astype(np.float32)

    ra, a = f32(rng.standard_normal(na)), f32(rng.standard_normal(na))
    rt, t = (f32(rng.standard_normal(nt)), f32(rng.standard_normal(nt))) if nt else (None, None)
    mu, lv = f32(3 * rng.standard_normal(nl)), f32(rng.uniform(-12, 6, nl))
    sums_ref, *grads_ref = OO.loss_sums_and_grads(ra, a, rt, t, mu, lv, COEF)
    bounds = grad_bounds(grads_ref[0], grads_ref[1], grads_ref[2], lv, COEF[2])
    lv64, mu64 = lv.astype(np.float64), mu.astype(np.float64)
    sum_bounds = (4 * U * sums_ref[0], 4 * U * sums_ref[1],
                  8 * U * float(np.sum(1 + np.abs(lv64) + mu64 ** 2 + np.exp(lv64))))

    dev = {k: (None if x is None else torch.from_numpy(x).to(cuda)) for k, x in
           dict(ra=ra, a=a, rt=rt, t=t, mu=mu, lv=lv).items()}
    coef = torch.tensor(COEF, dtype=torch.float32, device=cuda)
    lib = L.lib()
    ws = torch.empty(int(lib.hlmc_loss_workspace(na, nt, nl)), dtype=torch.uint8, device=cuda)
    assert ws.numel() >= 24
    outs = []
    for fused in (False, True):
        sums = torch.full((3,), float("nan"), dtype=torch.float64, device=cuda)
        d = {k: torch.full((n + SPARE,), SENT, device=cuda)
             for k, n in (("ra", na), ("rt", nt), ("mu", nl), ("lv", nl))}
        drt = d["rt"].data_ptr() if nt else None
        if fused:
            L.check(lib.hlmc_loss_sums_backward(L.stream(), L.ptr(dev["ra"]), L.ptr(dev["a"]), na, d["ra"].data_ptr(),
                                                L.ptr(dev["rt"]), L.ptr(dev["t"]), nt, drt, L.ptr(dev["mu"]),
                                                L.ptr(dev["lv"]), nl, coef.data_ptr(), d["mu"].data_ptr(),
                                                d["lv"].data_ptr(), sums.data_ptr(), ws.data_ptr()),
                    "hlmc_loss_sums_backward")
        else:
            L.check(lib.hlmc_loss_sums(L.stream(), L.ptr(dev["ra"]), L.ptr(dev["a"]), na, L.ptr(dev["rt"]),
                                       L.ptr(dev["t"]), nt, L.ptr(dev["mu"]), L.ptr(dev["lv"]), nl, sums.data_ptr(),
                                       ws.data_ptr()), "hlmc_loss_sums")
            L.check(lib.hlmc_loss_backward(L.stream(), L.ptr(dev["ra"]), L.ptr(dev["a"]), na, d["ra"].data_ptr(),
                                           L.ptr(dev["rt"]), L.ptr(dev["t"]), nt, drt, L.ptr(dev["mu"]),
                                           L.ptr(dev["lv"]), nl, coef.data_ptr(), d["mu"].data_ptr(),
                                           d["lv"].data_ptr()), "hlmc_loss_backward")
        torch.cuda.synchronize()
        outs.append((sums.cpu().numpy(), *(d[k].cpu().numpy() for k in ("ra", "rt", "mu", "lv"))))
    for x, y in zip(*outs):
        assert np.array_equal(x, y), "fused and separate entry points differ"
    sums, dra, drt, dmu, dlv = outs[1]
    for k, n in ((dra, na), (drt, nt), (dmu, nl), (dlv, nl)):
        assert np.all(k[n:] == SENT), "wrote past the end"
    rs = [abs(sums[k] - sums_ref[k]) / sum_bounds[k] if sum_bounds[k] else float(sums[k] != sums_ref[k])
          for k in range(3)]
    rg = [ratio(dra[:na], grads_ref[0], bounds[0]), ratio(drt[:nt], grads_ref[1], bounds[1]) if nt else 0.0,
          ratio(dmu[:nl], grads_ref[2], bounds[2]), ratio(dlv[:nl], grads_ref[3], bounds[3])]
    print("loss kernels worst |err| / bound: sums " + " ".join(f"{r:.3f}" for r in rs) + "  dra drt dmu dlv "
          + " ".join(f"{r:.3f}" for r in rg))
    assert max(rs) <= 1.0, rs
    assert max(rg) <= 1.0, rg


# scalars of the returned (total, l_audio, l_text, kld) to differentiate, with their upstream gradients
SCALARS = {"total": (1.0, 0.0, 0.0, 0.0), "la+3kld": (0.0, 1.0, 0.0, 3.0), "lt": (0.0, 0.0, 1.0, 0.0),
           "0.5total-la": (0.5, -1.0, 0.0, 0.0)}
B, HW, TD, LD = 3, (16, 24), 5, 7


@pytest.fixture(scope="module")
def loss_inputs():
    g = torch.Generator().manual_seed(21)
    return dict(ra=torch.randn(B, 1, *HW, generator=g), a=torch.randn(B, 1, *HW, generator=g),
                rt=torch.randn(B, TD, generator=g), t=torch.randn(B, TD, generator=g),
                mu=3 * torch.randn(B, LD, generator=g), lv=torch.rand(B, LD, generator=g) * 18 - 12)


# "lt" only where the loss has a text term
CASES = [(w, s) for w in ("hybrid", "hybrid_audio_only", "cvae", "simple") for s in SCALARS
         if s != "lt" or w in ("hybrid", "cvae")]


@pytest.mark.parametrize("which,scalar", CASES)
def test_loss_wrappers_match_float64_autograd(cuda, loss_inputs, which, scalar):
    """loss_function (with and without the text term), cvae_loss_function and vae_loss: every member of the tuple
    within 1e-6 relative of the float64 oracle's, and the gradients of four different scalars of the tuple within
    the kernel bounds, the mixed upstream coefficient standing in for ca / ct / ck."""
    has_text = which in ("hybrid", "cvae")
    gT, gA, gX, gK = SCALARS[scalar]
    beta = {"hybrid": 0.7, "hybrid_audio_only": 0.7, "cvae": 4.0, "simple": 0.8}[which]
    x = loss_inputs
    nl = x["mu"].numel()

    def leaves(dtype, dev):
        names = ("ra", "rt", "mu", "lv") if has_text else ("ra", "mu", "lv")
        return {k: x[k].to(dev, dtype).requires_grad_() for k in names}

    def call(fns, lf, tgt):
        if which == "simple":
            total, la, kl = fns.vae_loss(lf["ra"], tgt["a"], lf["mu"], lf["lv"], beta=beta)
            return total, la, None, kl
        if which == "cvae":
            return fns.cvae_loss_function(lf["ra"], tgt["a"], lf["rt"], tgt["t"], lf["mu"], lf["lv"], beta=beta)
        return fns.loss_function(lf["ra"], tgt["a"], lf.get("rt"), tgt["t"] if has_text else None, lf["mu"], lf["lv"],
                                 beta=beta)

    def scalar_of(tup):
        s = gT * tup[0] + gA * tup[1] + gK * tup[3]
        return s + gX * tup[2] if has_text else s

    ref_leaves = leaves(torch.float64, "cpu")
    ref = call(OM, ref_leaves, {k: v.double() for k, v in x.items()})
    scalar_of(ref).backward()
    our_leaves = leaves(torch.float32, cuda)
    ours = call(hlmc_amd, our_leaves, {k: v.to(cuda) for k, v in x.items()})
    scalar_of(ours).backward()
    torch.cuda.synchronize()

    for k, (o, r) in enumerate(zip(ours, ref)):
        if o is None:
            continue
        assert o.dtype == torch.float32 and o.dim() == 0
        o, r = float(o.detach()), float(r.detach())
        assert abs(o - r) <= 1e-6 * abs(r), (k, o, r)
    ck = beta * gT + gK
    if which == "simple":
        ck /= nl

    def gnp(t, like):
        return np.zeros(like.shape) if t.grad is None else t.grad.detach().double().cpu().numpy()

    refs = {k: gnp(ref_leaves[k], x[k]) for k in ref_leaves}
    bounds = grad_bounds(refs["ra"], refs.get("rt"), refs["mu"], x["lv"].numpy(), ck)
    bounds = dict(ra=bounds[0], rt=bounds[1], mu=bounds[2], lv=bounds[3])
    rs = {}
    for k in our_leaves:
        assert our_leaves[k].grad is not None, k
        rs[k] = ratio(gnp(our_leaves[k], x[k]), refs[k], bounds[k])
    print(f"{which} d({scalar}) worst |err| / bound: " + " ".join(f"{k} {r:.3f}" for k, r in rs.items()))
    assert max(rs.values()) <= 1.0, rs
