"""Sums of the counters of one kernel over a rocprofv3 --pmc --output-format csv directory, and per launch.
Usage: pmc_kernel_sum.py PMC_DIR OUT.json KERNEL_NAME_PART (profiles/NOTES_r18.md: the r18_pmc_stream_*.json files)."""
import csv, glob, json, sys, collections
d, out, kern = sys.argv[1], sys.argv[2], sys.argv[3]
acc = collections.defaultdict(float); rows = collections.defaultdict(int)
for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if kern in r["Kernel_Name"]:
            acc[r["Counter_Name"]] += float(r["Counter_Value"]); rows[r["Counter_Name"]] += 1
res = {"kernel": kern, "launches": max(rows.values()) if rows else 0, **{k: v for k, v in sorted(acc.items())}}
for k in list(acc):
    res[k + "_per_launch"] = round(acc[k] / max(rows[k], 1), 1)
json.dump(res, open(out, "w"), indent=1)
print(out, json.dumps(res))
