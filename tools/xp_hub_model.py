"""CPU model of the count hop's hub short cut (profiles/NOTES_xp_hub.md): the top hub of the bench graph, the share of the
entries of A' in its out-rows, the share of a label's live sources that reach it in exactly two hops, and the passes of a
whole-frontier scan that hold such sources only once the live list is ordered strong-first and classed as
spgemm.hip expand_count_scan does.  And of the second reduced plan (profiles/NOTES_xp_hub_set.md): the hub set H — the rows with at
least a quarter of the top hub's out-degree, at most 32, by (degree descending, id ascending) — the share of the entries of A' in
the union of its out-rows, the share of the live sources that reach ALL of H in exactly two hops, and per label the passes of
tier-A rows only (second plan), of strong rows only (first plan) and the others (full plan).
Usage: xp_hub_model.py [SCALE] [OUT.json] [OUT_SET.json]"""
import json
import sys

import numpy as np

import oracle

I64, U64 = np.int64, np.uint64
SCAN_KMAX, PASS_ROWS = 5, 1024


SET_DEG_DEN, SET_MAX, SET_MIN_SHARE_DEN = 4, 32, 8


def main(scale, out, out_set=""):
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
    # the hub set and what every vertex reaches of it in one hop (bit i: an edge to H[i]), in two (the OR over its out-row)
    q = np.nonzero(outdeg >= -(-int(outdeg[h]) // SET_DEG_DEN))[0]
    hubs = [int(x) for x in q[np.lexsort((q, -outdeg[q]))][:SET_MAX]]
    assert hubs[0] == h
    in_union = np.zeros(n, dtype=bool)
    mask1 = np.zeros(n, dtype=np.uint32)
    for i, x in enumerate(hubs):
        in_union[v[rowptr[x]:rowptr[x + 1]]] = True
        mask1[u[v == x]] |= np.uint32(1 << i)
    full = np.uint32((1 << len(hubs)) - 1) if len(hubs) < 32 else np.uint32(0xFFFFFFFF)
    mask2 = np.zeros(n, dtype=np.uint32)
    has_out = outdeg > 0
    mask2[has_out] = np.bitwise_or.reduceat(mask1[v], rowptr[:-1][has_out])
    union_share = int(indeg[in_union].sum()) / nnz
    builds = len(hubs) >= 2 and (union_share - share) * SET_MIN_SHARE_DEN >= 1.0
    res2 = {"scale": scale, "entries": nnz, "hubs": hubs, "hub_out_degrees": [int(outdeg[x]) for x in hubs],
            "third_tier_out_degree": int(np.sort(outdeg)[-len(hubs) - 1]), "union_rows": int(in_union.sum()),
            "top_hub_share_of_entries": round(share, 4), "union_share_of_entries": round(union_share, 4),
            "second_plan_built": bool(builds), "labels": []}
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
        # three tiers: A (all of H), B (the top hub, not all), weak; a pass of A rows only runs under the second plan
        tier_a = mask2[live] == full
        cls_a = tier_a[one][first]
        ma, deep, strong_only = m[cls_a], 0, 0
        for k, rows in enumerate(rows_of(kmax)):
            a_rows = (0 if k else int((tier_a & ~one).sum())) + int((((ma >> k) & 1) if k < kmax else (ma >> kmax)).sum())
            s_rows = (0 if k else plain_strong) + int((((ms >> k) & 1) if k < kmax else (ms >> kmax)).sum())
            for first_row in range(0, rows, PASS_ROWS):
                end = min(first_row + PASS_ROWS, rows)
                deep += 1 if end <= a_rows else 0
                strong_only += 1 if a_rows < end <= s_rows else 0
        res2["labels"].append({"class": c, "live": len(live), "tier_a_share": round(float(tier_a.mean()), 4),
                               "tier_b_share": round(float((st & ~tier_a).mean()), 4), "passes": passes_of(kmax),
                               "tier_a_passes": deep, "tier_b_passes": strong_only, "full_passes": passes_of(kmax) - deep - strong_only})
        print(res2["labels"][-1], flush=True)
    print({k: x for k, x in res.items() if k != "labels"})
    print({k: x for k, x in res2.items() if k != "labels"})
    if out:
        json.dump(res, open(out, "w"), indent=1)
    if out_set:
        json.dump(res2, open(out_set, "w"), indent=1)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 22, sys.argv[2] if len(sys.argv) > 2 else "",
         sys.argv[3] if len(sys.argv) > 3 else "")
