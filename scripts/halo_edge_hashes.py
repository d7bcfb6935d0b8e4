"""SHA-256 of every output of the LDS halo-tile kernels (csrc/halo.hpp) on seeded inputs, op by op: the four bench
shapes at B = 256 and the edge shapes of tests/test_ops_gpu.py (HALO_EDGE), each in the plain, statistics and
input-BatchNorm forms.  Run once per library and diff the two files: a refactor of the kernels must leave every line
as it was.
    HLMC_LIB=<parent libhlmc.so> python scripts/halo_edge_hashes.py parent.txt
    python scripts/halo_edge_hashes.py new.txt && diff parent.txt new.txt"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hlmc_amd  # noqa: E402,F401
from hlmc_amd import _lib as L  # noqa: E402

dev = torch.device("cuda")
lib, P = L.lib(), L.ptr
WS = 64 << 20
ws = torch.empty(WS, dtype=torch.uint8, device=dev)
# (kind 0 conv_s2 / 1 subpixel, B, Hi, Wi, Ci, Co)
SHAPES = [(0, 64, 64, 32, 64), (0, 32, 32, 64, 128), (1, 32, 32, 64, 32), (1, 16, 16, 128, 64)]
CASES = [(k, 256, h, w, ci, co) for k, h, w, ci, co in SHAPES] + [
    (0, 1, 8, 64, 32, 64), (0, 1, 8, 32, 64, 128), (1, 1, 4, 32, 64, 32), (1, 1, 8, 16, 128, 64),
    (0, 257, 8, 64, 32, 64), (0, 65, 16, 32, 64, 128), (1, 257, 8, 32, 64, 32), (1, 65, 16, 16, 128, 64)]


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
for kind, B, Hi, Wi, Ci, Co in CASES:
    g = torch.Generator().manual_seed(kind * 1000 + B + Hi + Ci)
    x = (torch.randn(B, Hi, Wi, Ci, generator=g) * (torch.rand(Ci, generator=g) + 0.5)).to(torch.bfloat16).to(dev)
    wp = (torch.randn(Co, 3, 3, Ci, generator=g) / (3 * Ci ** 0.5)).to(torch.bfloat16).to(dev)
    b = (torch.randn(Co, generator=g) * 0.1).to(dev)
    gamma, beta = (1 + 0.1 * torch.randn(Ci, generator=g)).to(dev), (0.1 * torch.randn(Ci, generator=g)).to(dev)
    oshape = (B, Hi // 2, Wi // 2, Co) if kind == 0 else (B, 2 * Hi, 2 * Wi, Co)
    tag = f"kind {kind} B={B} {Hi}x{Wi} {Ci}->{Co}"
    y = torch.zeros(*oshape, dtype=torch.bfloat16, device=dev)
    op = lib.hlmc_op_conv_s2 if kind == 0 else lib.hlmc_op_subpixel
    L.check(op(L.stream(), L.HLMC_BF16, P(x), B, Hi, Wi, Ci, P(wp), P(b), Co, P(y), P(ws), WS))
    print(f"{tag} plain: y {digest(y)}", file=out)
    wsb = int(lib.hlmc_op_halo_workspace(Ci, Co))
    for bn_in in (False, True):
        y.zero_()
        rm, rv = torch.full((Ci,), 0.25, device=dev), torch.full((Ci,), 1.5, device=dev)
        nbt = torch.zeros(1, dtype=torch.int64, device=dev)
        mean, inv = torch.zeros(Ci, device=dev), torch.zeros(Ci, device=dev)
        a_out = torch.zeros(B, Hi, Wi, Ci, dtype=torch.bfloat16, device=dev)
        sums = torch.zeros(2 * Co, dtype=torch.float64, device=dev)
        L.check(lib.hlmc_op_halo_fwd(L.stream(), kind, P(x), B, Hi, Wi, Ci, P(wp), P(b), Co, P(y), P(sums),
                                     P(gamma) if bn_in else None, P(beta) if bn_in else None, P(rm), P(rv), P(nbt),
                                     0.1, 1e-5, P(mean), P(inv), P(a_out), P(ws), wsb), "hlmc_op_halo_fwd")
        torch.cuda.synchronize()
        names = dict(y=y, out_sums=sums, mean=mean, invstd=inv, running_mean=rm, running_var=rv, nbt=nbt, a_out=a_out)
        print(f"{tag} {'bn_in+stats' if bn_in else 'stats'}: " + " ".join(f"{k} {digest(v)}" for k, v in names.items()),
              file=out)
