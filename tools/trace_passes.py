"""Splits a one-lane rocprofv3 kernel trace of bench.py into passes (scan_pass_kernel opens one) and count hops, and says which hops
took a hub short cut and at which level: bp_hub_sums_kernel<2> ran (the hub set's plan), bp_hub_sums_kernel<1> — or the untemplated
kernel of an older build — ran (the top hub's plan), or neither (the full plan).  Usage: trace_passes.py TRACE_DIR OUT.json"""
import csv, glob, json, re, sys
import numpy as np

d, out = sys.argv[1], sys.argv[2]
rows = []
for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"].replace("void ", "")
        m = re.search(r"(?:fgpu::)?(\w+)\s*(?:<|\()", name)
        k = m.group(1) if m else r["Kernel_Name"][:60]
        if k == "bp_hub_sums_kernel":
            k = "bp_hub_sums_kernel<2>" if re.search(r"bp_hub_sums_kernel<\s*2\s*>", name) else "bp_hub_sums_kernel<1>"
        rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, k))
rows.sort()
passes, cur = [], None
for t, us, k in rows:
    if k == "scan_pass_kernel":
        cur = {"us": 0.0, "level": 0, "stream": None, "fold": None, "zero": None, "plain_count": None, "n": 0}
        passes.append(cur)
    if cur is None:
        continue
    cur["us"] += us
    cur["n"] += 1
    if k == "bp_hub_sums_kernel<2>":
        cur["level"] = 2
    elif k == "bp_hub_sums_kernel<1>":
        cur["level"] = 1
    elif k == "xp_stream_kernel":
        cur["stream"] = us
    elif k in ("xp_fold_pieces_kernel", "xp_fold_kernel"):
        cur["fold"] = us
    elif k == "xp_zero_rows_kernel":
        cur["zero"] = us
    elif k == "bp_pull_kernel" and us > 500:
        cur["plain_count"] = us


def pct(v):
    v = np.array([x for x in v if x is not None])
    if not len(v):
        return None
    return {"n": len(v), "p10": round(float(np.percentile(v, 10)), 1), "p50": round(float(np.percentile(v, 50)), 1),
            "p90": round(float(np.percentile(v, 90)), 1), "mean": round(float(v.mean()), 1)}


res = {"passes": len(passes)}
for name, sel in (("hub_set", [p for p in passes if p["level"] == 2]), ("saturated", [p for p in passes if p["level"] == 1]),
                  ("full", [p for p in passes if not p["level"] and p["stream"] is not None]),
                  ("not_partitioned", [p for p in passes if p["stream"] is None])):
    res[name] = {"passes": len(sel), "pass_kernel_us": pct([p["us"] for p in sel]), "xp_stream_kernel": pct([p["stream"] for p in sel]),
                 "xp_fold": pct([p["fold"] for p in sel]), "xp_zero_rows_kernel": pct([p["zero"] for p in sel]),
                 "plain_count_pull": pct([p["plain_count"] for p in sel])}
# the unsaturated passes one by one: kernel time, stream, fold, plain count pull
res["unsaturated_list"] = [[round(p["us"], 1), p["stream"] and round(p["stream"], 1), p["fold"] and round(p["fold"], 1),
                            p["plain_count"] and round(p["plain_count"], 1)] for p in passes if not p["level"]]
res["all_pass_us_sum_ms"] = round(sum(p["us"] for p in passes) / 1e3, 2)
json.dump(res, open(out, "w"), indent=1)
print(out, json.dumps({k: v for k, v in res.items() if k != "unsaturated_list"}))
