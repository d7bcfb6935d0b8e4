"""SHA-256 of every output of the GEMM launchers (csrc/gemm_ops.hip) and their split-K reduce kernels (csrc/gemm.hpp) on
seeded inputs, op by op: every case of test_conv_s2, test_subpixel_convT, test_wgrad_s2_conv, test_linear,
test_linear_relu_mask and test_linear_wgrad (tests/test_ops_gpu.py) in both dtypes, and the bench shapes at B = 256 in
bf16.  The workspace queries the C ABI exposes (hlmc_net_workspace_bytes, which sums the ops' split-K workspaces over a
net's layers, and hlmc_op_halo_workspace) are printed first: they need no GPU (`--ws-only`).  Run once per library and
diff the two files: a refactor of the launchers or the reduces must leave every line as it was.
    HLMC_LIB=<parent libhlmc.so> python scripts/gemm_reduce_hashes.py parent.txt
    python scripts/gemm_reduce_hashes.py new.txt && diff parent.txt new.txt"""
import ctypes as C
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hlmc_amd  # noqa: E402,F401
from hlmc_amd import _lib as L  # noqa: E402

lib, P = L.lib(), L.ptr
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out = open(args[0], "w") if args else sys.stdout

# ---- workspace queries (host only)
NETS = [("hybrid 128x128 text 768", L.NET_HYBRID, [128, 768, 128, 128]),
        ("hybrid 128x128 audio only", L.NET_HYBRID, [128, 0, 128, 128]),
        ("hybrid 128x1024 text 768", L.NET_HYBRID, [128, 768, 128, 1024]),
        ("cvae 128x128", L.NET_CVAE, [128, 768, 10, 128, 128]),
        ("simple 370", L.NET_SIMPLE, [370, 32, 2, 256, 128])]
for name, kind, cfg in NETS:
    for dname, code in (("fp32", L.HLMC_F32), ("bf16", L.HLMC_BF16)):
        h = C.c_void_p()
        L.check(lib.hlmc_net_create(kind, L.i64_array(cfg), len(cfg), code, C.byref(h)), "hlmc_net_create")
        sizes = " ".join(f"B={b}:{int(lib.hlmc_net_workspace_bytes(h, b))}" for b in (1, 2, 3, 4, 7, 16, 32, 64, 100, 256, 512))
        print(f"ws net {name} {dname}: {sizes}", file=out)
        lib.hlmc_net_destroy(h)
for ci, co in ((32, 64), (64, 128), (64, 32), (128, 64)):
    print(f"ws halo {ci}->{co}: {int(lib.hlmc_op_halo_workspace(ci, co))}", file=out)

# ... and the ops' own queries behind them (csrc/ops.hpp; the library exports them under their C++ names), per shape
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_ops_gpu as T  # noqa: E402


def cases(test):  # the parametrize lists of tests/test_ops_gpu.py, read from the test functions themselves
    marks = [m for m in getattr(T, test).pytestmark if m.name == "parametrize" and m.args[0] != "dt"]
    return list(marks[0].args[1])


def ops_ws(name, dname, *a):
    fn = getattr(lib, f"_ZN4hlmc3ops{len(name)}{name}I{'f' if dname == 'fp32' else '14__hip_bfloat16'}EEm{'i' * len(a)}")
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int] * len(a)
    return f"ws {name} {dname} {a}: {fn(*a)}"


BENCH = [(256,) + c for c in T.BENCH_CONV], [(256,) + c for c in T.BENCH_SUBPIXEL], [(256,) + c for c in T.BENCH_WGRAD]
for dname in ("fp32", "bf16"):
    for B, Hi, Wi, Ci, Co in cases("test_conv_s2") + BENCH[0]:
        print(ops_ws("conv_s2_ws", dname, B, Hi, Wi, Ci, Co), file=out)
    for B, Hi, Wi, Ci, Co in cases("test_subpixel_convT") + BENCH[1]:
        print(ops_ws("subpixel_ws", dname, B, Hi, Wi, Ci, Co), file=out)
    for B, Hl, Wl, M, Cc in cases("test_wgrad_s2_conv") + BENCH[2]:
        print(ops_ws("wgrad_s2_ws", dname, B, Hl, Wl, M, Cc), file=out)
    for M, K, N in sorted({(c[0], c[1], c[2]) for c in cases("test_linear") + cases("test_linear_relu_mask")}):
        print(ops_ws("linear_ws", dname, M, K, N), file=out)
        print(ops_ws("linear_partials_ws", dname, M, K, N), file=out)
    for Mb, N, K in cases("test_linear_wgrad"):
        print(ops_ws("linear_wgrad_ws", dname, Mb, N, K), file=out)
if "--ws-only" in sys.argv:
    sys.exit(0)

dev = torch.device("cuda")
WS = 512 << 20
ws = torch.empty(WS, dtype=torch.uint8, device=dev)
DT = {"fp32": (L.HLMC_F32, torch.float32), "bf16": (L.HLMC_BF16, torch.bfloat16)}


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def conv(kind, dt, B, Hi, Wi, Ci, Co, g):
    code, tdt = DT[dt]
    x = torch.randn(B, Hi, Wi, Ci, generator=g).to(dev, tdt)
    wp = (torch.randn(Co, 3, 3, Ci, generator=g) / (3 * Ci ** 0.5)).to(dev, tdt)
    b = torch.randn(Co, generator=g).to(dev)
    y = torch.zeros((B, Hi // 2, Wi // 2, Co) if kind == 0 else (B, 2 * Hi, 2 * Wi, Co), dtype=tdt, device=dev)
    op = lib.hlmc_op_conv_s2 if kind == 0 else lib.hlmc_op_subpixel
    L.check(op(L.stream(), code, P(x), B, Hi, Wi, Ci, P(wp), P(b), Co, P(y), P(ws), WS))
    return f"y {digest(y)}"


def wgrad(dt, B, Hl, Wl, M, Cc, g):
    code, tdt = DT[dt]
    dy = torch.randn(B, Hl, Wl, M, generator=g).to(dev, tdt)
    x = torch.randn(B, 2 * Hl, 2 * Wl, Cc, generator=g).to(dev, tdt)
    dW = torch.zeros(M, Cc, 3, 3, device=dev)
    L.check(lib.hlmc_op_wgrad_s2(L.stream(), code, P(dy), B, Hl, Wl, M, P(x), Cc, P(dW), P(ws), WS))
    return f"dW {digest(dW)}"


def linear(dt, M, K, N, ldx, act, acc, mask, g):
    code, tdt = DT[dt]
    ldw = ((K + 7) // 8) * 8
    x = torch.randn(M, ldx, generator=g).to(dev, tdt)
    w = torch.zeros(N, ldw)
    w[:, :K] = torch.randn(N, K, generator=g) / K ** 0.5
    w = w.to(dev, tdt)
    b = torch.randn(N, generator=g).to(dev)
    y = torch.randn(M, N, generator=g).to(dev, tdt)
    ref = torch.randn(M, N, generator=g).clamp_min(0).to(dev, tdt) if mask else None
    L.check(lib.hlmc_op_linear(L.stream(), code, P(x), ldx, M, K, P(w), ldw, None if mask else P(b), N, P(y), N, act, acc,
                               0, P(ws), WS, P(ref)))
    return f"y {digest(y)}"


def linear_wgrad(dt, Mb, N, K, g):
    code, tdt = DT[dt]
    ldd, ldx = ((N + 7) // 8) * 8, ((K + 7) // 8) * 8
    dy = torch.randn(Mb, ldd, generator=g).to(dev, tdt)
    x = torch.randn(Mb, ldx, generator=g).to(dev, tdt)
    res = []
    for with_bias in (False, True):
        dW, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        L.check(lib.hlmc_op_linear_wgrad(L.stream(), code, P(dy), ldd, P(x), ldx, Mb, N, K, P(dW),
                                         P(db) if with_bias else None, P(ws), WS))
        res.append(f"dW {digest(dW)} db {digest(db)}")
    return " | ".join(res)


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


for dt in ("fp32", "bf16"):
    for c in cases("test_conv_s2"):
        print(f"conv_s2 {dt} {c}: {conv(0, dt, *c, gen(0, *c))}", file=out)
    for c in cases("test_subpixel_convT"):
        print(f"subpixel {dt} {c}: {conv(1, dt, *c, gen(1, *c))}", file=out)
    for c in cases("test_wgrad_s2_conv"):
        print(f"wgrad_s2 {dt} {c}: {wgrad(dt, *c, gen(2, *c))}", file=out)
    for M, K, N, ldx, act, acc in cases("test_linear"):
        print(f"linear {dt} {(M, K, N, ldx, act, acc)}: {linear(dt, M, K, N, ldx, act, acc, False, gen(3, M, K, N, acc))}",
              file=out)
    for M, K, N, acc in cases("test_linear_relu_mask"):
        print(f"linear_relu_mask {dt} {(M, K, N, acc)}: {linear(dt, M, K, N, K, 0, acc, True, gen(4, M, K, N, acc))}",
              file=out)
    for c in cases("test_linear_wgrad"):
        print(f"linear_wgrad {dt} {c}: {linear_wgrad(dt, *c, gen(5, *c))}", file=out)
for Hi, Wi, Ci, Co in T.BENCH_CONV:
    print(f"conv_s2 bf16 B=256 {(Hi, Wi, Ci, Co)}: {conv(0, 'bf16', 256, Hi, Wi, Ci, Co, gen(6, Hi, Ci))}", file=out)
for Hi, Wi, Ci, Co in T.BENCH_SUBPIXEL:
    print(f"subpixel bf16 B=256 {(Hi, Wi, Ci, Co)}: {conv(1, 'bf16', 256, Hi, Wi, Ci, Co, gen(7, Hi, Ci))}", file=out)
for Hl, Wl, M, Cc in T.BENCH_WGRAD:
    print(f"wgrad_s2 bf16 B=256 {(Hl, Wl, M, Cc)}: {wgrad('bf16', 256, Hl, Wl, M, Cc, gen(8, Hl, M))}", file=out)
torch.cuda.synchronize()
