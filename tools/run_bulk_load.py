"""One bulk load of the RAW R-MAT tuples of a scale (repeated pairs included) through the host layer — the workload to put
under a profiler (rocprofv3 --kernel-trace --stats -- python tools/run_bulk_load.py 22).  Prints what the load did."""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import oracle
from falkordb_amd import host

scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
u, v = oracle.rmat_edges(scale)
ids = np.arange(len(u), dtype=np.uint64)
hc = host.Context(0)
g = host.Graph(hc, 1 << scale)
t = g.add_type("KNOWS")
t0 = time.perf_counter()
st = g.bulk_insert_edges(t, u, v, ids)
dt = time.perf_counter() - t0
print(json.dumps({"scale": scale, "tuples": len(u), "s": round(dt, 3), "stats": st,
                  "host_phases_ms": {k: round(x, 2) for k, x in g.last_bulk_phases_ms().items()}}))
del g
hc.close()
