"""Resource table of every kernel in a hipcc object or shared library: VGPRs, AGPRs, SGPRs, scratch bytes, LDS bytes and
the waves per EU the registers allow (gfx950: 512 unified VGPRs per lane, allocated in blocks of 8, at most 8 waves), one
line per kernel sorted by demangled name, from the code object's metadata note.  No GPU needed.
    python scripts/kernel_resources.py build/gemm_ops.hip.o [name-filter ...] > table.txt
Diff two tables to see what a refactor did to the code objects.  With --summary, the kernels named by a filter are
listed one by one without their argument lists and every other kernel template is one line: the number of
instantiations, the range of each figure, and a SHA-256 over the template's full per-kernel lines.  Equal digests in two
summaries mean every instantiation has the same name and the same figures in both."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
ARCH = os.environ.get("ARCH", "gfx950")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def main():
    summary = "--summary" in sys.argv
    obj, *filters = [a for a in sys.argv[1:] if a != "--summary"]
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
        run(f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "copy"))
        run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={co}",
            f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}")
        notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
    rows = []
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        f = {k: v for k, v in re.findall(r"\.(\w+):\s+'?([^\n']+)'?", ".agpr_count:" + blk.split("\namdhsa.target")[0])}
        name = f["name"]
        regs = int(f["vgpr_count"])  # the unified count (architectural + accumulation registers)
        waves = min(8, 512 // max(8, -(-regs // 8) * 8))
        rows.append((name, regs, int(f["agpr_count"]), int(f["sgpr_count"]), int(f["private_segment_fixed_size"]),
                     int(f["group_segment_fixed_size"]), waves))
    names = run("c++filt", *[r[0] for r in rows]).splitlines()
    print("vgpr agpr sgpr scratch lds waves/EU  kernel")
    groups = {}
    for dn, r in sorted(zip(names, rows)):
        dn = dn.replace("void ", "", 1)
        listed = not filters or any(x in dn for x in filters)
        fig = f"{r[1]:4d} {r[2]:4d} {r[3]:4d} {r[4]:7d} {r[5]:6d} {r[6]:3d}"
        if summary and not listed:
            groups.setdefault(re.split(r"[<(]", dn)[0], []).append((fig, dn))
        elif listed:
            print(f"{fig}  {re.sub(r'[(](?!anonymous namespace[)]).*$', '', dn) if summary else dn}")
    for base, ks in sorted(groups.items()):
        digest = hashlib.sha256("\n".join(f"{f}  {n}" for f, n in ks).encode()).hexdigest()[:16]
        cols = list(zip(*[[int(x) for x in f.split()] for f, _ in ks]))
        span = " ".join(f"{min(c)}..{max(c)}" for c in cols)
        print(f"{base}  x {len(ks)}  (ranges: {span})  sha256 {digest}")

main()
