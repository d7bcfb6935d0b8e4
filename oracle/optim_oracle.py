"""Float64 restatements of the training step's tail: one Adam step and the VAE loss sums with their gradients.

Plain numpy, written from the formulas (torch.optim.Adam's single-tensor, non-amsgrad, non-maximize update; the
include/hlmc.h loss contract), so the HIP kernels are compared with something that shares no code with them.
Inputs of any float type are promoted to float64; nothing is modified in place.
"""
from __future__ import annotations

import numpy as np


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def adam_step(p, g, m, v, lr, b1, b2, eps, wd, step):
    """New (p, m, v) after step number `step` (1-based) of torch.optim.Adam(lr, (b1, b2), eps, weight_decay=wd):

        g += wd p;  m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g^2
        p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
    """
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    lr, b1, b2, eps, wd, step = float(lr), float(b1), float(b2), float(eps), float(wd), int(step)
    if wd != 0.0:
        g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** step)
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
    return p - step_size * (m / denom), m, v


def loss_sums_and_grads(ra, a, rt, t, mu, lv, coef):
    """(sums, dra, drt, dmu, dlv) of the hlmc.h loss contract, for coef = (ca, ct, ck):

        sums = (sum (ra - a)^2, sum (rt - t)^2, sum (1 + lv - mu^2 - e^lv))
        dra = ca (ra - a);  drt = ct (rt - t);  dmu = ck mu;  dlv = -0.5 ck (1 - e^lv)

    rt / t may be None (no text term): sums[1] is 0 and drt is None.
    """
    ra, a, mu, lv = _f64(ra), _f64(a), _f64(mu), _f64(lv)
    ca, ct, ck = (float(c) for c in coef)
    da = ra - a
    e = np.exp(lv)
    s1, drt = 0.0, None
    if rt is not None:
        dt = _f64(rt) - _f64(t)
        s1 = float(np.sum(dt * dt))
        drt = ct * dt
    sums = np.array([np.sum(da * da), s1, np.sum(1.0 + lv - mu * mu - e)], dtype=np.float64)
    return sums, ca * da, drt, ck * mu, -0.5 * ck * (1.0 - e)
