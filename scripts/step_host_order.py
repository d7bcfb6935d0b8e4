"""One train step in the order the HOST issued it: every HIP call that puts work on a stream (kernel launches, memsets,
async copies, event records, event waits), each launch with its queue, grid and kernel.  From one rocprofv3 run with
--kernel-trace --hip-runtime-trace (csv); rows are ordered by correlation id, no timestamp enters the listing, so
two runs of one library give the same text (scripts/step_list.py's start order of concurrent queues does not).
    python scripts/step_host_order.py KERNEL_TRACE_CSV HIP_API_TRACE_CSV [STEP_FROM_END]"""
import csv
import sys

kern = {int(r["Correlation_Id"]): r for r in csv.DictReader(open(sys.argv[1]))}
api = sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Correlation_Id"]))
k = int(sys.argv[3]) if len(sys.argv) > 3 else 1
KEEP = ("Launch", "hipMemsetAsync", "hipMemcpyAsync", "hipMemcpyWithStream", "hipEventRecord", "hipStreamWaitEvent")
rows = [(r["Function"], kern.get(int(r["Correlation_Id"]))) for r in api if any(t in r["Function"] for t in KEEP)]
idx = [i for i, (_, kr) in enumerate(rows) if kr and "stft_mel" in kr["Kernel_Name"]]
queues = {}
for fn, kr in rows[idx[-k - 1]:idx[-k]]:
    if kr is None:
        print(fn)
        continue
    q = queues.setdefault(kr["Queue_Id"], f"Q{len(queues)}")
    n = kr["Kernel_Name"].replace("hlmc::", "").replace("(anonymous namespace)::", "").replace("__hip_bfloat16", "bf")
    n = n.replace("void ", "").split("(")[0][:70]
    g = int(kr["Grid_Size_X"]) // int(kr["Workgroup_Size_X"])
    print(f"{fn} {q} grid {g}x{kr['Grid_Size_Y']}x{kr['Grid_Size_Z']} {n}")
