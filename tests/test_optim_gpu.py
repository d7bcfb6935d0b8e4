"""The multi-tensor Adam kernel (hlmc_adam_step) and the Python optimizer on top of it (hlmc_amd.Adam).

hlmc_adam_step is compared, one step from identical float32 inputs, with oracle/optim_oracle.adam_step (numpy
float64) called with the hyper-parameters rounded to float32 -- the values that cross the C ABI.  The bounds are
rounding-count bounds in u = 2^-24, and a numpy float32 restatement of the kernel's operation order (adam_fp32
below) has to meet them on the CPU side of the same test before the GPU is asked to.

hlmc_amd.Adam is compared with torch.optim.Adam(foreach=False) on a float32 CPU copy fed the same gradients.
There the float32 betas matter: the kernel forms 1 - beta from the float32 beta, torch rounds the double 1 - beta,
so the moments differ from torch's by up to |float32(beta) - beta| / (1 - beta) relative (1.3e-5 for 0.999).
"""
import copy
import math

import numpy as np
import pytest
import torch

import hlmc_amd
from hlmc_amd import _lib as L
from oracle import optim_oracle as OO

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SIZES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
HYPER = [(1e-4, (.9, .999), 1e-8, 0.0, 1), (1e-3, (.9, .999), 1e-8, 1e-2, 3), (1e-2, (.5, .9), 1e-3, 0.1, 1000),
         (1e-3, (0.0, .999), 1e-8, 0.0, 100000)]


def f32_hyper(lr, betas, eps, wd):
    """The hyper-parameters as the C ABI receives them: rounded to float32, returned as Python doubles."""
    return tuple(float(np.float32(x)) for x in (lr, betas[0], betas[1], eps, wd))


def adam_fp32(p, g, m, v, lr, b1, b2, eps, wd, step):
    """adam_val of csrc/kernels.hip in numpy float32, operation for operation (no contraction; the step size and
    sqrt(1 - b2^step) come from the host in double and are rounded once, as adam_coef does)."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    step_size = f(float(lr) / (1.0 - float(b1) ** step))
    bc2_sqrt = f(math.sqrt(1.0 - float(b2) ** step))
    gi = g + wd * p if wd != 0 else g
    mi = m + (gi - m) * (f(1) - b1)
    vi = v * b2 + ((f(1) - b2) * gi) * gi
    denom = np.sqrt(vi) / bc2_sqrt + eps
    pn = p - step_size * (mi / denom)
    assert pn.dtype == mi.dtype == vi.dtype == f
    return pn, mi, vi


def adam_bounds(p, g, m, v, lr, b1, b2, eps, wd, step, cancelling=False):
    """(reference (p, m, v), elementwise bounds on |dp|, |dm|, |dv|) for one float32 Adam step, hyper-parameters
    already rounded to float32.  With s = lr / (1 - b1^step), c = sqrt(1 - b2^step), D = sqrt(v_ref) / c + eps:

        |dm| <= 4u sm,  sm = |m| + |g| + wd |p|
        |dv| <= 8u v_ref + 1e-37
        |dp| <= 4u (|p| + |upd| + s sm / D)

    cancelling: g + wd p may cancel (gradients a model produced).  Its float32 value is then off by
    dg = 2u (|g| + wd |p|), which is no longer small against the sum, so
      * v_ref in the v bound is taken at |g| + wd |p| in place of g + wd p;
      * the denominator is only known to lie above D_lo = sqrt(max(v_ref - e, 0)) / c + eps with
        e = (1 - b2) (2 |g + wd p| dg + dg^2), the shift of v under dg: s sm / D becomes s sm / D_lo, and the
        update moves by up to s |m_ref| dD / (D D_lo), dD = (sqrt(v_ref + e) - sqrt(max(v_ref - e, 0))) / c,
        on top of the roundings counted above.
    Where nothing cancels, e <= 4u v_ref and this is the first form with 8u |upd| in place of 4u |upd|."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    pr, mr, vr = OO.adam_step(p, g, m, v, lr, b1, b2, eps, wd, step)
    big = np.abs(g) + wd * np.abs(p)
    sm = np.abs(m) + big
    s = lr / (1.0 - b1 ** step)
    c = math.sqrt(1.0 - b2 ** step)
    upd = np.abs(p - pr)
    d_ref = np.sqrt(vr) / c + eps
    if not cancelling:
        return (pr, mr, vr), (4 * U * (np.abs(p) + upd + s * sm / d_ref), 4 * U * sm, 8 * U * vr + 1e-37)
    dg = 2 * U * big
    e = (1.0 - b2) * (2 * np.abs(g + wd * p) * dg + dg * dg)
    lo = np.sqrt(np.maximum(vr - e, 0.0))
    d_lo = lo / c + eps
    bp = 4 * U * (np.abs(p) + upd + s * sm / d_lo) + s * np.abs(mr) * ((np.sqrt(vr + e) - lo) / c) / (d_ref * d_lo)
    return (pr, mr, vr), (bp, 4 * U * sm, 8 * U * (v * b2 + (1.0 - b2) * big * big) + 1e-37)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 counts as 0: an exact result under a zero bound)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def kernel_inputs(wd, step, seed):
    """70 tensors (three kAdamMax batches) of sizes around the kernel's 1024-element block and 256-thread stride;
    magnitudes over several decades, exact zeros in g, g given the sign of p under weight decay (no cancellation in
    g + wd p), zero moments at step 1 and random ones (v >= 0) later."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(70):
        n = SIZES[k % len(SIZES)]

        def mag(lo, hi):
            return (10.0 ** rng.uniform(lo, hi, n)) * rng.choice([-1.0, 1.0], n)

        p = mag(-4, 1)
        g = mag(-6, 2)
        g[rng.random(n) < 0.05] = 0.0
        if wd != 0:
            g = np.abs(g) * np.sign(p)
        if step == 1:
            m, v = np.zeros(n), np.zeros(n)
        else:
            m, v = mag(-6, 2), mag(-6, 2) ** 2
        out.append(tuple(x.astype(np.float32) for x in (p, g, m, v)))
    return out


@pytest.mark.parametrize("lr,betas,eps,wd,step", HYPER)
def test_adam_kernel_matches_float64(cuda, lr, betas, eps, wd, step):
    """One hlmc_adam_step over 70 tensors against the float64 restatement, within the rounding bounds of
    adam_bounds; spare elements behind every tensor untouched; a second call from the same inputs bit-identical.
    Measured on MI355X, worst |err| / bound over the four cases: p 0.59, m 0.48, v 0.60 (2.4u, 1.9u, 4.8u), the
    same figures as the float32 restatement's: the kernel and the restatement agreed in every printed digit."""
    hp = f32_hyper(lr, betas, eps, wd)
    data = kernel_inputs(wd, step, seed=step)
    refs = [adam_bounds(*t, *hp, step) for t in data]
    # the reference arithmetic itself (float32, kernel order) meets the bounds
    worst_cpu = [0.0, 0.0, 0.0]
    for t, (ref, bnd) in zip(data, refs):
        for k, got in enumerate(adam_fp32(*t, *hp, step)):
            worst_cpu[k] = max(worst_cpu[k], worst_ratio(got, ref[k], bnd[k]))
    print(f"adam_fp32 (CPU) worst |err| / bound: p {worst_cpu[0]:.3f} m {worst_cpu[1]:.3f} v {worst_cpu[2]:.3f}")
    assert max(worst_cpu) <= 1.0, worst_cpu

    SENT, SPARE = -12345.5, 8

    def run():
        bufs = []
        for t in data:
            row = []
            for x in t:
                b = torch.full((x.size + SPARE,), SENT, dtype=torch.float32)
                b[:x.size] = torch.from_numpy(x)
                row.append(b.to(cuda))
            bufs.append(row)
        arrs = [L.vp_array([row[k].data_ptr() for row in bufs]) for k in range(4)]
        L.check(L.lib().hlmc_adam_step(L.stream(), len(bufs), arrs[0], arrs[1], arrs[2], arrs[3],
                                       L.i64_array([t[0].size for t in data]), lr, betas[0], betas[1], eps, wd, step,
                                       None), "hlmc_adam_step")
        torch.cuda.synchronize()
        return [[b.cpu() for b in row] for row in bufs]

    first, second = run(), run()
    worst = [0.0, 0.0, 0.0]
    for t, (ref, bnd), row, row2 in zip(data, refs, first, second):
        n = t[0].size
        for k, b in enumerate(row):
            assert torch.all(b[n:] == SENT), "wrote past numel"
            assert torch.equal(b, row2[k]), "second call differs"
        assert np.array_equal(row[1][:n].numpy(), t[1]), "gradient modified"
        for k, j in enumerate((0, 2, 3)):
            worst[k] = max(worst[k], worst_ratio(row[j][:n].numpy(), ref[k], bnd[k]))
    print(f"hlmc_adam_step worst |err| / bound: p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst


def beta_slack(b):
    """Relative deviation of a moment from torch's allowed for the float32 beta of the C ABI (the kernel's
    1.f - float32(b) against torch's float32(1 - b)), twice over, plus 16 u of rounding."""
    return 16 * U + 2 * abs(float(np.float32(b)) - b) / (1 - b)


def test_adam_optimizer_matches_torch(cuda):
    """hlmc_amd.Adam against torch.optim.Adam(foreach=False) on a float32 CPU copy, 4 steps of fed gradients:
    two groups with their own lr / weight_decay, a parameter without a gradient on step 2 (step counts diverge,
    one step() issues two launches for its group), a non-contiguous gradient, a group added after step 1; then the
    two optimizers exchange state_dicts and take one more step.  Parameters: the suite's rtol 1e-6 / atol 1e-7
    (atol scaled by lr / 1e-4); moments: beta_slack (exp_avg relative to |m| + |g|, exp_avg_sq to itself).
    Measured on MI355X: exp_avg at 0.39 of its bound, exp_avg_sq at 0.498 of 2.67e-5, i.e. 1.33e-5 relative -- the
    float32-beta2 term at its derived size, before and after the exchange."""
    g = torch.Generator().manual_seed(9)
    shapes = {"a": (33, 65), "b": (257,), "c": (40, 48), "d": (1025,)}
    cpu = {k: torch.randn(s, generator=g).requires_grad_() for k, s in shapes.items()}
    gpu = {k: v.detach().clone().to(cuda).requires_grad_() for k, v in cpu.items()}
    g0, g1, g2 = dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-3, weight_decay=1e-2), dict(lr=1e-2, weight_decay=0.1)

    def groups(ps):
        return [dict(params=[ps["a"], ps["b"]], **g0), dict(params=[ps["c"]], **g1)]

    opt_t = torch.optim.Adam(groups(cpu), foreach=False)
    opt_h = hlmc_amd.Adam(groups(gpu))
    worst = {"exp_avg": 0.0, "exp_avg_sq": 0.0}

    def one_step(k, names):
        for n in cpu:
            cpu[n].grad = gpu[n].grad = None
        for n in names:
            gr = torch.randn(shapes[n], generator=g) * (0.1 if n == "a" else 1.0)
            if n in "cd":  # weight decay: g takes the sign of p, or g + wd p cancels and two correct float32
                # evaluations (torch's fused multiply-add, the kernel's two roundings) differ without bound in v
                gr = torch.where(cpu[n].detach() >= 0, gr.abs(), -gr.abs())
            if n == "c":  # a transposed view: same values, non-contiguous on the GPU side
                gpu[n].grad = gr.t().contiguous().to(cuda).t()
                assert not gpu[n].grad.is_contiguous()
            else:
                gpu[n].grad = gr.to(cuda)
            cpu[n].grad = gr.clone()
        opt_t.step()
        opt_h.step()
        torch.cuda.synchronize()

    def compare(tag):
        for gt, gh in zip(opt_t.param_groups, opt_h.param_groups):
            lr, wd, (b1, b2) = gt["lr"], gt["weight_decay"], gt["betas"]
            assert (gh["lr"], gh["weight_decay"], tuple(gh["betas"])) == (lr, wd, (b1, b2))
            for pt, ph in zip(gt["params"], gh["params"]):
                torch.testing.assert_close(ph.detach().cpu(), pt.detach(), rtol=1e-6, atol=1e-7 * lr / 1e-4, msg=tag)
                st, sh = opt_t.state[pt], opt_h.state[ph]
                assert bool(st) == bool(sh), tag
                if not st:
                    continue
                assert int(st["step"]) == int(sh["step"]), tag
                gi = np.abs(pt.grad.numpy().astype(np.float64)) if pt.grad is not None else 0.0
                m, v = st["exp_avg"].double().numpy(), st["exp_avg_sq"].double().numpy()
                em = np.abs(sh["exp_avg"].cpu().double().numpy() - m) / (np.abs(m) + gi)
                ev = np.abs(sh["exp_avg_sq"].cpu().double().numpy() - v) / v
                worst["exp_avg"] = max(worst["exp_avg"], float(em.max()) / beta_slack(b1))
                worst["exp_avg_sq"] = max(worst["exp_avg_sq"], float(ev.max()) / beta_slack(b2))
                assert float(em.max()) <= beta_slack(b1), (tag, float(em.max()))
                assert float(ev.max()) <= beta_slack(b2), (tag, float(ev.max()))

    one_step(1, ["a", "b", "c"])
    compare("step 1")
    opt_t.add_param_group(dict(params=[cpu["d"]], **g2))
    opt_h.add_param_group(dict(params=[gpu["d"]], **g2))
    one_step(2, ["a", "c", "d"])      # b has no gradient: its step count stays at 1
    compare("step 2")
    one_step(3, ["a", "b", "c", "d"])
    one_step(4, ["a", "b", "c", "d"])
    compare("step 4")
    steps = [int(opt_h.state[gpu[n]]["step"]) for n in "abcd"]
    assert steps == [4, 3, 4, 3]
    print(f"vs torch, 4 steps: worst exp_avg {worst['exp_avg']:.3f} exp_avg_sq {worst['exp_avg_sq']:.3f} of the bound"
          f" (exp_avg_sq bound {beta_slack(0.999):.3e})")

    # the interchange the optim.py docstring promises: each side continues from the other's state_dict
    sd_t, sd_h = copy.deepcopy(opt_t.state_dict()), copy.deepcopy(opt_h.state_dict())
    opt_h.load_state_dict(sd_t)
    opt_t.load_state_dict(sd_h)
    for n in "abcd":
        assert opt_h.state[gpu[n]]["exp_avg"].is_cuda and not opt_t.state[cpu[n]]["exp_avg"].is_cuda
    one_step(5, ["a", "b", "c", "d"])
    compare("after state_dict exchange")
    assert [int(opt_h.state[gpu[n]]["step"]) for n in "abcd"] == [5, 4, 5, 4]
    print(f"after exchange: worst exp_avg {worst['exp_avg']:.3f} exp_avg_sq {worst['exp_avg_sq']:.3f} of the bound")
