"""What tests/exact_cases.py's two checks catch and the relative L2 norm over the whole tensor does not, shown on the
CPU with float32 torch ops on the bf16-rounded operands as the stand-in for the kernels (f32 accumulation, one
rounding to the output dtype): the stand-in passes both checks unmodified, and each seeded fault

    tap     one tap dropped at one corner pixel, all channels            conv_s2 (3, 64, 64, 32 -> 64), bf16
    ulp2    one output element two bf16 ulp off                          the same conv
    term    one weight-gradient element missing one (b, r, c) term       wgrad_s2 (16, 8, 8, 128, 128), B Hl Wl = 1024
    slab    one split-K slab of one 64 x 64 tile added twice             linear (4, 16384, 1024), bf16: plan_nt's
                                                                         16 tiles x 32 slabs of 512
    kterm   one product of 16384 dropped from one element                the same linear

fails assert_exact on integer operands.  assert_elementwise (random data) resolves tap, ulp2, term and slab; kterm is
below it: one product of a K = 16384 sum is ~1/128 against a bound of (K + 16) 2^-23 absref ~ 0.16 (a single dropped
term is under the K u bound once K exceeds about 2900), which is why the exact form exists.

The gap: tap, ulp2, term and kterm keep the relative L2 error under the limit the GPU test of that op uses
(tests/test_ops_gpu.py: 1e-2 bf16 outputs, 5e-3 bf16 weight gradients).  slab does not: plan_nt splits until
tiles x slabs ~ 512 blocks, so one doubled slab of one tile moves the norm by ~1 / sqrt(512) = 4.4e-2 of the product's
norm on uniform data (measured here with the bias in the norm: 3.3e-2), above the 1e-2 limit; the norm sees that one,
the per-element checks name its tile."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_cases as X

BF16, F32 = torch.bfloat16, torch.float32
L2_BF16, L2_WGRAD_BF16 = 1e-2, 5e-3   # tests/test_ops_gpu.py: DT["bf16"], the bf16 weight gradients

CONV = (3, 64, 64, 32, 64)            # in exact_cases.CONV_S2 / HALO shapes' layer, B = 3
SUBPIXEL = (2, 16, 16, 128, 64)
WGRAD = (16, 8, 8, 128, 128)
LINEAR = (4, 16384, 1024)             # exact_cases.LINEAR_RELU_MASK's K = 16384 product
LINEAR_WGRAD = (300, 8, 8)
SLAB_TILE, SLAB_K = (0, 1), (5 * 512, 6 * 512)   # tile (row 0, col 1) of 64 x 64; slab 5 of 32


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(b.norm(), 1e-30))


def bq(t):  # operands as the bf16 kernels see them
    return t.to(BF16).to(torch.float64)


# the ops on NHWC operands of any float dtype (float32: the stand-in kernel; float64: the reference)
def conv_s2(x, w, b):
    return F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1).permute(0, 2, 3, 1)


def subpixel(x, w, b):
    return F.conv_transpose2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)


def wgrad_s2(x, dy):
    return torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (dy.shape[3], x.shape[3], 3, 3),
                                       dy.permute(0, 3, 1, 2), stride=2, padding=1)


def linear(x, w, b):
    return x @ w.T + b


def linear_wgrad(dy, x):
    return dy.T @ x


def operands(family, exact, seed=0):
    """float64 operands of the family's shape: integers (exact) or bf16-rounded normals scaled as in test_ops_gpu."""
    g = torch.Generator().manual_seed(seed + 17)

    def data(shape, scale=1.0, extra=False):
        if exact:
            return X.int_operands(g, shape, -X.EXTRA_MAX, X.EXTRA_MAX) if extra else X.int_operands(g, shape)
        t = torch.randn(*shape, generator=g) * scale
        return t.double() if extra else bq(t)   # bias is f32 on the device

    if family == "conv_s2":
        B, Hi, Wi, Ci, Co = CONV
        return data((B, Hi, Wi, Ci)), data((Co, Ci, 3, 3), 1 / (3 * Ci ** 0.5)), data((Co,), extra=True)
    if family == "subpixel":
        B, Hi, Wi, Ci, Co = SUBPIXEL
        return data((B, Hi, Wi, Ci)), data((Ci, Co, 3, 3), 1 / (3 * Ci ** 0.5)), data((Co,), extra=True)
    if family == "wgrad_s2":
        B, Hl, Wl, M, C = WGRAD
        return data((B, 2 * Hl, 2 * Wl, C)), data((B, Hl, Wl, M))
    if family == "linear":
        M, K, N = LINEAR
        return data((M, K)), data((N, K), K ** -0.5), data((N,), extra=True)
    Mb, N, K = LINEAR_WGRAD
    return data((Mb, N)), data((Mb, K))


FAMILY = {  # op, k_terms of the shape, output dtype of the bf16 kernel, L2 limit of its GPU test
    "conv_s2": (conv_s2, 9 * CONV[3], BF16, L2_BF16),
    "subpixel": (subpixel, 9 * SUBPIXEL[3], BF16, L2_BF16),
    "wgrad_s2": (wgrad_s2, WGRAD[0] * WGRAD[1] * WGRAD[2], F32, L2_WGRAD_BF16),
    "linear": (linear, LINEAR[1], BF16, L2_BF16),
    "linear_wgrad": (linear_wgrad, LINEAR_WGRAD[0], F32, L2_WGRAD_BF16),
}
_cache = {}


def case(family, exact):
    """(operands, float32 stand-in result before the output rounding, float64 reference, absref); computed once."""
    if (family, exact) not in _cache:
        op = FAMILY[family][0]
        ops = operands(family, exact)
        _cache[family, exact] = (ops, op(*(t.float() for t in ops)), op(*ops), op(*(t.abs() for t in ops)))
    ops, y32, ref, absref = _cache[family, exact]
    return ops, y32.clone(), ref, absref


# ---- the seeded faults: each edits the float32 stand-in result in place and returns the coordinate it touched
def drop_tap(ops, y32):
    x, w, _ = ops
    b, kh, kw = 1, 1, 1    # output pixel (0, 0) of image 1 reads input (2 oh - 1 + kh, 2 ow - 1 + kw) = (0, 0)
    y32[b, 0, 0, :] -= (w[:, :, kh, kw] @ x[b, 0, 0, :]).float()
    return "b 1, row 0, col 0, channel"


def drop_wgrad_term(ops, y32):
    x, dy = ops
    b, r, c, kh, kw = 9, 3, 4, 2, 0
    # the position's largest product (never a zero one, which would be no fault): |dy x| ~ 5 with the random data,
    # against a bound of (1024 + 16) 2^-23 absref ~ 0.08 -- a typical product of ~0.4 is resolved as well
    m, ci = int(dy[b, r, c].abs().argmax()), int(x[b, 2 * r - 1 + kh, 2 * c - 1 + kw].abs().argmax())
    y32[m, ci, kh, kw] -= float(dy[b, r, c, m] * x[b, 2 * r - 1 + kh, 2 * c - 1 + kw, ci])
    return f"m {m}, c {ci}, kh {kh}, kw {kw}"


def double_slab(ops, y32):
    x, w, _ = ops
    (tr, tc), (k0, k1) = SLAB_TILE, SLAB_K
    y32[64 * tr:64 * tr + 64, 64 * tc:64 * tc + 64] += (x[:, k0:k1] @ w[64 * tc:64 * tc + 64, k0:k1].T).float()
    return "tile (0, 1) of 64 x 64"


def drop_k_term(ops, y32):
    x, w, _ = ops
    m, n, k = 2, 700, 9001
    if float(x[m, k] * w[n, k]) == 0:   # integer operands: a zero product is no fault; the next one that is not
        k = int((x[m] * w[n]).nonzero()[0])
    y32[m, n] -= float(x[m, k] * w[n, k])
    return "row 2, col 700"


def two_ulp(y):  # on the rounded bf16 output: two steps of the bf16 encoding at one element
    y.view(torch.int16)[1, 5, 7, 3] += 2
    return "b 1, row 5, col 7, channel 3"


MUTATIONS = {  # family, fault on the f32 result, fault on the rounded output, assert_elementwise resolves it, L2 gap
    "tap": ("conv_s2", drop_tap, None, True, True),
    "ulp2": ("conv_s2", None, two_ulp, True, True),
    "term": ("wgrad_s2", drop_wgrad_term, None, True, True),
    "slab": ("linear", double_slab, None, True, False),
    "kterm": ("linear", drop_k_term, None, False, True),
}
WGRAD_AXES = ("m", "c", "kh", "kw")


def mutated(name, exact):
    family, pre, post, _, _ = MUTATIONS[name]
    ops, y32, ref, absref = case(family, exact)
    where = pre(ops, y32) if pre else None
    got = y32.to(FAMILY[family][2])
    if post:
        where = post(got)
    return family, got, ref, absref, where


@pytest.mark.parametrize("family", list(FAMILY))
def test_stand_in_passes_both_checks(family):
    op, k_terms, out_dtype, limit = FAMILY[family]
    X.check_budget(k_terms, 2 * X.EXTRA_MAX)
    _, y32, ref, _ = case(family, True)
    assert float(ref.abs().max()) < X.TWO24
    X.assert_exact(y32.to(out_dtype), ref, out_dtype, family)
    _, y32, ref, absref = case(family, False)
    ratio = X.assert_elementwise(y32.to(out_dtype), ref, absref, k_terms, out_dtype, family)
    assert ratio <= 1.0 and rel(y32.to(out_dtype), ref) < limit


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_exact_check_fails_every_mutation_and_names_it(name):
    family, got, ref, _, where = mutated(name, True)
    axes = WGRAD_AXES if family == "wgrad_s2" else None
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got, ref, FAMILY[family][2], name, tile=(64, 64), axes=axes)
    print(e.value)
    assert where in str(e.value), str(e.value)


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_elementwise_check_fails_what_its_bound_resolves(name):
    family, got, ref, absref, where = mutated(name, False)
    _, k_terms, out_dtype, _ = FAMILY[family]
    if MUTATIONS[name][3]:
        with pytest.raises(AssertionError, match="outside the per-element bound"):
            X.assert_elementwise(got, ref, absref, k_terms, out_dtype, name)
    else:   # one product of K = 16384: under the K u bound
        assert X.assert_elementwise(got, ref, absref, k_terms, out_dtype, name) <= 1.0


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_l2_norm_of_each_mutation_against_todays_limit(name):
    """The gap, written down: with the random data of tests/test_ops_gpu.py these faults stay under the relative L2
    limit of their op's test.  The doubled slab is the exception (module docstring): ~1 / sqrt(tiles x slabs)."""
    family, got, ref, _, _ = mutated(name, False)
    clean = rel(case(family, False)[1].to(FAMILY[family][2]), ref)
    e = rel(got, ref)
    print(f"{name}: rel L2 {clean:.2e} clean, {e:.2e} with the fault; limit {FAMILY[family][3]:.0e}")
    if MUTATIONS[name][4]:
        assert e < FAMILY[family][3]
    else:
        assert FAMILY[family][3] < e < 0.1


def test_every_exact_shape_stays_in_the_exact_f32_range():
    budgets = X.exact_case_budgets()
    assert len(budgets) > 100
    for what, budget in budgets:
        assert budget < X.TWO24, (what, budget)
    assert max(b for _, b in budgets) == 262144 * 4   # the 32 x 32 weight gradient at B = 256
    with pytest.raises(AssertionError):
        X.check_budget(2 ** 22 + 1)                   # 4 (2^22 + 1) >= 2^24


def test_int_operands_are_integers_in_range():
    t = X.int_operands(torch.Generator().manual_seed(1), (1000,))
    assert t.dtype == torch.float64 and bool((t == t.round()).all())
    assert sorted(set(t.tolist())) == [-2.0, -1.0, 0.0, 1.0, 2.0]
    t = X.int_operands(torch.Generator().manual_seed(1), (1000,), -8, 8)
    assert float(t.min()) == -8 and float(t.max()) == 8


def test_elementwise_check_rejects_nan_and_nonzero_where_bound_is_zero():
    ref = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    absref = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    assert X.assert_elementwise(ref.float(), ref, absref, 4, F32, "clean") == 0.0
    for bad in ([[float("nan"), 0.0]], [[1.0, 1e-30]]):
        with pytest.raises(AssertionError):
            X.assert_elementwise(torch.tensor(bad), ref, absref, 4, F32, "bad")
