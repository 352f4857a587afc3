"""CPU model of the count hop's hub short cut (profiles/NOTES_xp_hub.md): the top hub of the bench graph, the share of the
entries of A' in its out-rows, the share of a label's live sources that reach it in exactly two hops, and the passes of a
whole-frontier scan that hold such sources only once the live list is ordered strong-first and classed as
spgemm.hip expand_count_scan does.  Usage: xp_hub_model.py [SCALE] [OUT.json]"""
import json
import sys

import numpy as np

import oracle

I64, U64 = np.int64, np.uint64
SCAN_KMAX, PASS_ROWS = 5, 1024


def main(scale, out):
    u, v = oracle.rmat_edges(scale)
    n = 1 << scale
    key = np.unique(u.astype(U64) << U64(32) | v.astype(U64))
    u, v = (key >> U64(32)).astype(I64), (key & U64(0xFFFFFFFF)).astype(I64)
    nnz = len(key)
    outdeg, indeg = np.bincount(u, minlength=n), np.bincount(v, minlength=n)
    h = int(np.argmax(outdeg))
    out_h = v[u == h]
    share = int(indeg[out_h].sum()) / nnz
    in_h = np.zeros(n, dtype=bool)
    in_h[u[v == h]] = True
    strong_v = np.zeros(n, dtype=bool)                       # some out-neighbour has an edge to h
    strong_v[u[in_h[v]]] = True
    rowptr = np.concatenate([[0], np.cumsum(outdeg)])
    res = {"scale": scale, "entries": nnz, "hub": h, "hub_out_degree": int(outdeg[h]), "rows_with_entries": int((indeg > 0).sum()),
           "hub_rows_share_of_rows": round(len(out_h) / int((indeg > 0).sum()), 4), "hub_rows_share_of_entries": round(share, 4), "labels": []}
    ids = np.arange(n, dtype=U64)
    hsh = oracle.mix64(ids) % U64(16)
    for c in range(16):
        src = ids[hsh == U64(c)].astype(I64)
        live = src[outdeg[src] > 0]
        st = strong_v[live]
        one = outdeg[live] == 1
        target = v[rowptr[live[one]]]
        _, first, m = np.unique(target, return_index=True, return_counts=True)
        cls_strong = st[one][first]
        nplain, plain_strong = int((~one).sum()), int((st & ~one).sum())
        bits = [int(((m >> k) & 1).sum()) for k in range(SCAN_KMAX + 1)]
        top = [int((m >> k).sum()) for k in range(SCAN_KMAX + 1)]
        rows_of = lambda kmax: [(0 if k else nplain) + (bits[k] if k < kmax else top[k]) for k in range(kmax + 1)]
        passes_of = lambda kmax: sum(-(-r // PASS_ROWS) for r in rows_of(kmax))
        kmax = min(range(SCAN_KMAX + 1), key=lambda k: (passes_of(k), k))
        ms = m[cls_strong]
        sat = 0
        for k, rows in enumerate(rows_of(kmax)):
            s_rows = (0 if k else plain_strong) + int((((ms >> k) & 1) if k < kmax else (ms >> kmax)).sum())
            sat += s_rows // PASS_ROWS + (1 if s_rows == rows and rows % PASS_ROWS > 64 else 0)
        res["labels"].append({"class": c, "sources": len(src), "live": len(live), "strong_share": round(float(st.mean()), 4),
                              "strong_share_deg_gt_1": round(float(st[~one].mean()), 4), "kmax": kmax, "passes": passes_of(kmax),
                              "saturated_passes": sat})
        print(res["labels"][-1], flush=True)
    print({k: x for k, x in res.items() if k != "labels"})
    if out:
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 22, sys.argv[2] if len(sys.argv) > 2 else "")
