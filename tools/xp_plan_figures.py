"""The count hop's partitioned plan at RMAT-22 (the bench graph), read back with fgpu_mat_xp_chunks under both cuts: chunks,
shared rows, and entries over the gather slots the stream kernel issues with and without its look-ahead.
Usage: xp_plan_figures.py OUT.json (profiles/r18_plan_figures.json)."""
import json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import bench
from falkordb_amd import engine
ctx = engine.Context(0)
A, dp, dm, _ = bench.khop_inputs(ctx, 22, 16)
out = {}
for cut in (0, 1):
    ctx.set_option("expand_xp_cut", cut)
    t = A.xp_chunks()
    lens = []
    for k in range(8):
        c0, c1 = int(t["cbase"][k]), int(t["cbase"][k + 1])
        st = np.concatenate([t["cstart"][c0:c1].astype(np.int64), [int(t["pstart"][k + 1])]])
        lens.append(np.diff(st))
    lens = np.concatenate(lens)
    its = (lens + 127) // 128
    out[cut] = {"cut_held": t["cut"], "chunks": int(len(lens)), "shared_rows": int(t["cshared"].sum()), "entries": int(lens.sum()),
                "mean_entries": round(float(lens.mean()), 1), "slots_no_lookahead": int((its * 128 + 64).sum()), "slots_lookahead": int((its * 128).sum()),
                "iterations_hist": {int(k): int(v) for k, v in zip(*np.unique(its, return_counts=True))}}
    out[cut]["entries_over_slots_no_lookahead"] = round(out[cut]["entries"] / out[cut]["slots_no_lookahead"], 4)
    out[cut]["entries_over_slots_lookahead"] = round(out[cut]["entries"] / out[cut]["slots_lookahead"], 4)
json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out))
ctx.close()
