#!/usr/bin/env python3
"""Throughput of the plane-cut queries (include/mi355pt.h pt_cut_count / pt_cut_search): the persistent kernel
against the simple one-plane-per-thread kernel, and the search (count walk + scan + fill walk) against two calls of the count, kernels
alternating, on C2 (dragon-class, 871,414 triangles) and C4 (sponza-class interior, 262,144 triangles), each at build level 0 and 2.

Plane sets: one plane through each of the first 262,144 points of the three point sets of tools/pointquery_bench.py (surface, box, far),
with a fixed random unit normal per plane and a cubic window around the point, in device memory (torch tensors, zero-copy).  Per set
three window sizes, one common half-size per set, found by bisection on the first 16,384 planes so that the mean list length is about 1,
8 and 64 entries per plane; the lengths actually obtained are recorded (a set whose planes cut nothing at any size is recorded as it is).
Per set, size and kernel: the median over --reps launches (after one warm-up) of the launch time by events on the context's stream, of
  count   pt_cut_count
  search  pt_cut_search with a capacity that holds every entry (no host wait)
in Mplanes/s and, for the search, Mentries/s.  search_over_two_counts = ms(search) / (2 x ms(count)).  Beside each row, `box_yardstick`:
pt_box_count and pt_box_search (persistent) on the same windows -- the same walk without the plane test at a node, and with the box
query's leaf test.  The node test of this query costs roughly twice the box query's instructions per child and prunes the children the
plane misses; cut_over_box, the ratio of the two times, is the number that says whether a cheaper plane test is worth a follow-up.  Per
set and size: node records and triangles per plane, stack_drops and max_stack from one PT_CUT_STATS pass.  There is no gate: the query
has no predecessor.

Every (config, build level) runs in a child process of its own under a time limit (--limit seconds); the file is written after every
row ("complete": false until the last), so a run that is cut short leaves what it measured, and after a child that fails or runs out of
time nothing more is started.

    python tools/cut_bench.py [--reps 5] [--configs C2,C4] [--sets surface,box,far] [--limit 900] [--out profiles/cut_ab.json]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")       # the package's own default; recorded in the output

import pointquery_bench as pq  # noqa: E402

N_PLANES, N_CALIBRATE = 262144, 16384
TARGETS = (1, 8, 64)
NORMAL_SEED = 29


def records(torch, centres, normals, half):
    """(n, 12) PtCutPlane records on the device: the plane through each centre, the window centre +- half"""
    nrm = normals[: centres.shape[0]]
    d = (nrm * centres).sum(dim=1, keepdim=True)
    z = torch.zeros((centres.shape[0], 1), dtype=torch.float32, device=centres.device)
    return torch.cat([nrm, d, centres - half, z, centres + half, z], dim=1).contiguous()


def boxes_of(rec):
    """(n, 8) PtBox records: the windows"""
    return rec[:, 4:12].contiguous()


def total_of(torch, counts):
    return int(counts.view(torch.int32).sum(dtype=torch.int64).item())


def half_for(ctx, torch, centres, normals, target, extent):
    """The common half-size at which the first N_CALIBRATE planes have `target` entries on average (bisection in log h)."""
    sub = centres[:N_CALIBRATE]
    lo, hi = 1e-5 * extent, 16.0 * extent
    for _ in range(40):
        h = float(np.sqrt(lo * hi))
        mean = total_of(torch, ctx.cut_count(records(torch, sub, normals, h))) / N_CALIBRATE
        if mean < target:
            lo = h
        else:
            hi = h
    return float(np.float32(hi))


def load(path):
    with open(path) as f:
        return json.load(f)


def save(path, result):
    with open(path, "w") as f:
        json.dump(result, f, indent=1)


def run_rows(args, name, accel):
    """The child: the rows of one config at one build level, appended to the file after every row."""
    import torch
    rt = importlib.import_module("raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = load(args.out)
    result["device"] = torch.cuda.get_device_name(0)
    c = pq.CONFIGS[name]
    tris = rt.procedural_scene(c["kind"], c["n"], pq.SCENE_SEED)
    v = tris.reshape(-1, 3)
    extent = float((v.max(0) - v.min(0)).max())
    nrm = np.random.default_rng(NORMAL_SEED).normal(size=(N_PLANES, 3))
    normals = torch.from_numpy((nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)).cuda()
    sets = {k: torch.from_numpy(np.ascontiguousarray(p[:N_PLANES])).cuda() for k, p in pq.point_sets(tris, np.random.default_rng(pq.RNG_SEED)).items()
            if k in args.sets.split(",")}
    ctx = rt.Context(0)
    ctx.set_triangles(tris); ctx.build_bvh(accel)
    ctx.set_stream(stream.cuda_stream)                       # launches straight on torch's stream: the events time the kernels alone
    out = {}
    result["configs"]["%s_accel%d" % (name, accel)] = {"triangles": c["n"], "accel": accel, "extent": extent, "sets": out}
    for sname, centres in sets.items():
        n = centres.shape[0]
        for target in TARGETS:
            half = half_for(ctx, torch, centres, normals, target, extent)
            rec = records(torch, centres, normals, half)
            boxes = boxes_of(rec)
            total = total_of(torch, ctx.cut_count(rec))
            box_total = total_of(torch, ctx.box_count(boxes))
            cap, box_cap = total + 64, box_total + 64
            ms = {"count_persistent": [], "count_simple": [], "search_persistent": [], "search_simple": [], "box_count": [], "box_search": []}
            ref = None
            for rep in range(args.reps + 1):
                for kernel in ("persistent", "simple"):
                    simple = kernel == "simple"
                    t, counts = pq.timed(torch, stream, lambda: ctx.cut_count(rec, simple=simple))
                    if rep:
                        ms["count_" + kernel].append(t)
                    t, res = pq.timed(torch, stream, lambda: ctx.cut_search(rec, capacity=cap, simple=simple))
                    if rep:
                        ms["search_" + kernel].append(t)
                    got = [res[0]] + [x.view(torch.int32)[:total] for x in res[1:]]
                    if ref is None:
                        ref = got
                        assert int(res[0][-1]) == total and torch.equal(torch.diff(res[0]), counts.view(torch.int32).to(torch.int64)), "counts and offsets disagree"
                    else:
                        assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the kernels disagree"
                t, _ = pq.timed(torch, stream, lambda: ctx.box_count(boxes))
                if rep:
                    ms["box_count"].append(t)
                t, _ = pq.timed(torch, stream, lambda: ctx.box_search(boxes, capacity=box_cap))
                if rep:
                    ms["box_search"].append(t)
            ctx.cut_count(rec, stats=True)
            st = ctx.stats()
            ctx.box_count(boxes, stats=True)
            box_st = ctx.stats()
            med = {k: statistics.median(x) for k, x in ms.items()}
            key = "%s_%d" % (sname, target)
            ours = ("count_persistent", "count_simple", "search_persistent", "search_simple")
            out[key] = {"planes": n, "half_size": half, "half_size_in_extents": round(half / extent, 6), "entries": total,
                        "entries_per_plane": round(total / n, 3),
                        "ms": {k: round(med[k], 4) for k in ours},
                        "mplanes_per_s": {k: round(n / (med[k] * 1e3), 1) for k in ours},
                        "mentries_per_s": {k: round(total / (med[k] * 1e3), 1) for k in ("search_persistent", "search_simple")},
                        "persistent_over_simple": {w: round(med[w + "_simple"] / med[w + "_persistent"], 3) for w in ("count", "search")},
                        "search_over_two_counts": {k: round(med["search_" + k] / (2 * med["count_" + k]), 3) for k in ("persistent", "simple")},
                        "box_yardstick": {"entries": box_total, "entries_per_box": round(box_total / n, 3),
                                          "ms": {k: round(med["box_" + k], 4) for k in ("count", "search")},
                                          "cut_over_box": {k: round(med[k + "_persistent"] / med["box_" + k], 3) for k in ("count", "search")},
                                          "node_records_per_box": round(box_st["nodes_examined"] / n, 2),
                                          "triangles_per_box": round(box_st["tris_tested"] / n, 2)},
                        "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                        "stats": st,
                        "node_records_per_plane": round(st["nodes_examined"] / n, 2),
                        "triangles_per_plane": round(st["tris_tested"] / n, 2)}
            print(name, "accel", accel, key, json.dumps({k: out[key][k] for k in ("entries_per_plane", "mplanes_per_s", "persistent_over_simple", "search_over_two_counts", "box_yardstick")}),
                  "drops", st["stack_drops"], "max_stack", st["max_stack"], flush=True)
            save(args.out, result)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default=",".join(pq.CONFIGS))
    ap.add_argument("--sets", default="surface,box,far")
    ap.add_argument("--limit", type=int, default=900, help="seconds for one config at one build level")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_ab.json"))
    ap.add_argument("--rows", default=None, help="CONFIG,LEVEL: run these rows in this process (what the tool starts its children with)")
    args = ap.parse_args()
    if args.rows:
        name, accel = args.rows.split(",")
        return run_rows(args, name, int(accel))
    save(args.out, {"tool": "tools/cut_bench.py", "reps": args.reps, "planes": N_PLANES, "sets": args.sets,
                    "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "complete": False, "configs": {}})
    for name in args.configs.split(","):
        for accel in pq.ACCELS:
            cmd = [sys.executable, os.path.abspath(__file__), "--rows", "%s,%d" % (name, accel), "--reps", str(args.reps), "--sets", args.sets, "--out", args.out]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:                                      # a failure, a fault or the time limit: nothing more is started
                print("%s accel %d ended with status %d: stopping, %s holds the rows measured so far" % (name, accel, rc, args.out), flush=True)
                return rc
    result = load(args.out)
    result["complete"] = True
    save(args.out, result)
    print(json.dumps({n: {s: v["mplanes_per_s"]["search_persistent"] for s, v in c["sets"].items()} for n, c in result["configs"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
