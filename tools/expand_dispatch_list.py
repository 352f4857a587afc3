"""The kernel dispatches of every k-hop entry and chain end, for comparing two builds of libfgpu.so.

Run (a fresh process per library, FGPU_LIB names the one to load; nothing but the kernel trace is collected):

    rocprofv3 --kernel-trace --output-format csv -d OUT/a -o t -- python tools/expand_dispatch_list.py run OUT/a.json
    FGPU_LIB=/path/to/other/libfgpu.so rocprofv3 --kernel-trace --output-format csv -d OUT/b -o t -- \\
        python tools/expand_dispatch_list.py run OUT/b.json
    python tools/expand_dispatch_list.py compare OUT/a OUT/b OUT/a.json OUT/b.json

`run` makes the calls of tests/test_gpu_expand_ownership.py once each, in a fixed order, and writes a digest of every result and
the context's final device_bytes() (in_use, pooled: `pooled` is what the pools grew to, the peak of the run).  `compare` orders
each trace by dispatch id and compares (kernel, grid, workgroup, LDS bytes) position by position, then the two JSON files."""
import csv
import glob
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(out_path):
    from falkordb_amd import engine
    spec = importlib.util.spec_from_file_location("ownership", os.path.join(ROOT, "tests", "test_gpu_expand_ownership.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    ctx = engine.Context(0)
    g = t._Graph(ctx)
    digests = []

    def note(name, value):
        digests.append((name, hashlib.sha256(repr(t._plain(value)).encode()).hexdigest()))

    for mode in (1, 2, 0):
        for labelled in (False, True):
            for dirty in (False, True):
                lab = g.label if labelled else None
                tag = f"mode{mode} label{int(labelled)} dirty{int(dirty)}"
                with t.options(ctx, expand_mode=mode):
                    for hops in (2, 3):
                        m, dp, dm = g.layers(dirty, hops)
                        kw = dict(dp=dp, dm=dm, dst_label_bitmap=lab)
                        note(f"expand {tag} {hops}", engine.expand(ctx, g.src, m, **kw))
                        note(f"expand32 {tag} {hops}", engine.expand32(ctx, g.src, m, **kw))
                        note(f"expand_mat {tag} {hops}", t._expand_mat(ctx, g.src, m, **kw))
                        note(f"pairs {tag} {hops}", engine.expand_pairs(ctx, g.src, m, **kw))
                        note(f"pairs pinned {tag} {hops}", engine.expand_pairs(ctx, g.src, m, pinned_dest=g.pin, row_bits=32, **kw))
                        note(f"probe {tag} {hops}", engine.expand_probe(ctx, g.src, g.dst, m, **kw))
                        note(f"stream {tag} {hops}", t._stream(ctx, g.src, m, **kw))
                        note(f"stream unread {tag} {hops}", t._stream(ctx, g.src, m, read=False, **kw))
                        for fuse in (0, 1):
                            with t.options(ctx, expand_fuse_count=fuse):
                                note(f"count fuse{fuse} {tag} {hops}", engine.expand_count(ctx, g.src, m, **kw))
                                note(f"count bare fuse{fuse} {tag} {hops}", engine.expand_count(ctx, g.src, m, want_checksum=False, **kw))
                    m, dp, dm = g.layers(dirty, 3)
                    note(f"levels {tag}", engine.expand_levels(ctx, g.src, m, dp=dp, dm=dm, dst_label_bitmap=lab))
    for dirty in (False, True):
        m, dp, dm = g.layers(dirty, 3)
        # ONE lane here: with two, which lane takes which pass — and so the order of the dispatch ids — is a race
        with t.options(ctx, expand_scan_min=64, expand_scan_rows=64, expand_scan_lanes=1):
            for src in (g.src, g.live_src):
                for cs in (True, False):
                    note(f"scan dirty{int(dirty)} cs{int(cs)}", engine.expand_count(ctx, src, m, dp=dp, dm=dm, want_checksum=cs))
        for hops in (1, 2):
            m, dp, dm = g.layers(dirty, hops)
            note(f"trails dirty{int(dirty)} {hops}", engine.expand_trail_counts(ctx, g.live_src, m, dp=dp, dm=dm))
    m, dp, dm = g.layers(True, 2)
    try:
        engine.expand_trail_counts(ctx, g.live_src, m, dp=dp, dm=dm, weighted=True)
        note("weighted over pattern layers", "no error")
    except Exception as e:   # FGPU_INVALID, after the merged layers were built
        note("weighted over pattern layers", str(e))
    ctx.sync()
    in_use, pooled = ctx.device_bytes()
    with open(out_path, "w") as f:
        json.dump({"lib": os.environ.get("FGPU_LIB", "tree"), "in_use": in_use, "pooled": pooled, "digests": digests}, f, indent=1)
    print(json.dumps({"calls": len(digests), "in_use": in_use, "pooled": pooled}))


def dispatches(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    shape = [c for c in rows[0] if c.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size"))]
    return [(r["Kernel_Name"],) + tuple(r[c] for c in shape) for r in rows]


def compare(dir_a, dir_b, json_a, json_b):
    a, b = dispatches(dir_a), dispatches(dir_b)
    differing = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    ja, jb = json.load(open(json_a)), json.load(open(json_b))
    report = {"dispatches": [len(a), len(b)], "distinct_kernels": [len({x[0] for x in a}), len({x[0] for x in b})],
              "first_differing_position": differing[0] if differing else None, "differing_positions": len(differing),
              "results_equal": ja["digests"] == jb["digests"], "calls": len(ja["digests"]),
              "in_use": [ja["in_use"], jb["in_use"]], "pooled": [ja["pooled"], jb["pooled"]]}
    print(json.dumps(report))
    if differing:
        i = differing[0]
        print("a:", a[i], "\nb:", b[i])
    ok = not differing and len(a) == len(b) and report["results_equal"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        compare(*sys.argv[2:6])
