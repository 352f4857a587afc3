"""Per-kernel launch statistics of a rocprofv3 --kernel-trace --output-format csv directory: launches, mean, 10th / 50th / 90th
percentile in us and the sum in ms, the 14 kernels with the largest sums.  Usage: kernel_launch_stats.py TRACE_DIR OUT.json
(profiles/NOTES_r18.md: the r18*_kernel_stats.json files)."""
import csv, glob, json, re, sys, collections
import numpy as np
d, out = sys.argv[1], sys.argv[2]
acc = collections.defaultdict(list)
files = glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True)
for f in files:
    for r in csv.DictReader(open(f)):
        m = re.search(r"(?:fgpu::)?(\w+)\s*(?:<|\()", r["Kernel_Name"].replace("void ", ""))
        acc[m.group(1) if m else r["Kernel_Name"][:60]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
res = {"files": len(files)}
for k, v in sorted(acc.items(), key=lambda kv: -sum(kv[1]))[:14]:
    v = np.array(v)
    res[k] = {"n": len(v), "mean": round(float(v.mean()), 1), "p10": round(float(np.percentile(v, 10)), 1), "p50": round(float(np.percentile(v, 50)), 1),
              "p90": round(float(np.percentile(v, 90)), 1), "sum_ms": round(float(v.sum()) / 1e3, 2)}
json.dump(res, open(out, "w"), indent=1)
for k in ("xp_stream_kernel", "xp_zero_rows_kernel", "xp_fold_pieces_kernel", "bp_pull_groups_kernel"):
    print(out, k, res.get(k))
