#!/usr/bin/env python3
"""Throughput of the triangle-overlap queries (include/mi355pt.h pt_tri_count / pt_tri_search): the persistent
kernel against the simple one-triangle-per-thread kernel, and the search (count walk + scan + fill walk) against two calls of the count,
in one process, kernels alternating, on C2 (dragon-class, 871,414 triangles) and C4 (sponza-class interior, 262,144 triangles), each at
build level 0 and 2.

Caller triangle sets: one triangle around each of the first 262,144 points of the three point sets of tools/pointquery_bench.py (surface,
box, far), in device memory (torch tensors, zero-copy): centre + size x three fixed random offsets in [-1, 1]^3 per triangle.  Per set three
sizes, one common size per set, found by bisection on the first 16,384 triangles so that the mean list length is about 1, 8 and 64 entries
per caller triangle; the lengths actually obtained are recorded (a set whose triangles cut nothing at any size is recorded as it is).
Per set, size and kernel: the median over --reps launches (after one warm-up) of the launch time by events on the context's stream, of
  count   pt_tri_count
  search  pt_tri_search with a capacity that holds every entry (no host wait)
in Mtriangles/s and, for the search, Mentries/s.  search_over_two_counts = ms(search) / (2 x ms(count)).  Beside each row, `box_yardstick`:
pt_box_count and pt_box_search (persistent) on the same triangles' bounding boxes -- the same walk with the box query's leaf test, which
lists several times as much: what the leaf test of this query costs, and saves.  Per set and size: node records and triangles per caller
triangle, stack_drops and max_stack from one PT_TRI_STATS pass.  There is no gate: the query has no predecessor.  The rows of 8 and 64
entries away from the surface take caller triangles that span much of the scene and run at 0.1 Mtriangles/s and below: the whole tool
takes tens of minutes, and it writes its file after every row ("complete": false until the last), so a run that is cut short leaves what
it measured.

    python tools/tri_bench.py [--reps 5] [--configs C2,C4] [--out profiles/tri_ab.json]      (--out defaults to that file)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")       # the package's own default; recorded in the output

import pointquery_bench as pq  # noqa: E402

N_TRIS, N_CALIBRATE = 262144, 16384
TARGETS = (1, 8, 64)
SHAPE_SEED = 23


def callers(torch, centres, shape, size):
    """(n, 12) PtTri records on the device: centre + size x the triangle's three offsets"""
    v = centres[:, None, :] + size * shape[: centres.shape[0]]
    return torch.cat([v, torch.zeros((v.shape[0], 3, 1), dtype=torch.float32, device=v.device)], dim=2).reshape(-1, 12).contiguous()


def boxes_of(torch, rec):
    """(n, 8) PtBox records: the bounding boxes of the caller triangles"""
    v = rec.reshape(-1, 3, 4)[:, :, :3]
    z = torch.zeros((v.shape[0], 1), dtype=torch.float32, device=v.device)
    return torch.cat([v.min(1).values, z, v.max(1).values, z], dim=1).contiguous()


def total_of(torch, counts):
    return int(counts.view(torch.int32).sum(dtype=torch.int64).item())


def size_for(ctx, torch, centres, shape, target, extent):
    """The common size at which the first N_CALIBRATE caller triangles have `target` entries on average (bisection in log size)."""
    sub = centres[:N_CALIBRATE]
    lo, hi = 1e-5 * extent, 16.0 * extent
    for _ in range(40):
        s = float(np.sqrt(lo * hi))
        mean = total_of(torch, ctx.tri_count(callers(torch, sub, shape, s))) / N_CALIBRATE
        if mean < target:
            lo = s
        else:
            hi = s
    return float(np.float32(hi))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default=",".join(pq.CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_ab.json"))
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("raytracer-public_amd")
    stream = torch.cuda.current_stream()
    shape = torch.from_numpy((np.random.default_rng(SHAPE_SEED).random((N_TRIS, 3, 3)) * 2 - 1).astype(np.float32)).cuda()
    result = {"tool": "tools/tri_bench.py", "reps": args.reps, "device": torch.cuda.get_device_name(0), "caller_triangles": N_TRIS,
              "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "complete": False, "configs": {}}

    def save():                                              # after every row: a run that is cut short leaves what it measured
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
    for name in args.configs.split(","):
        c = pq.CONFIGS[name]
        tris = rt.procedural_scene(c["kind"], c["n"], pq.SCENE_SEED)
        v = tris.reshape(-1, 3)
        extent = float((v.max(0) - v.min(0)).max())
        sets = {k: torch.from_numpy(np.ascontiguousarray(p[:N_TRIS])).cuda() for k, p in pq.point_sets(tris, np.random.default_rng(pq.RNG_SEED)).items()}
        for accel in pq.ACCELS:
            ctx = rt.Context(0)
            ctx.set_triangles(tris); ctx.build_bvh(accel)
            ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
            out = {}
            result["configs"]["%s_accel%d" % (name, accel)] = {"triangles": c["n"], "accel": accel, "extent": extent, "sets": out}
            for sname, centres in sets.items():
                n = centres.shape[0]
                for target in TARGETS:
                    size = size_for(ctx, torch, centres, shape, target, extent)
                    rec = callers(torch, centres, shape, size)
                    boxes = boxes_of(torch, rec)
                    total = total_of(torch, ctx.tri_count(rec))
                    box_total = total_of(torch, ctx.box_count(boxes))
                    cap, box_cap = total + 64, box_total + 64
                    ms = {"count_persistent": [], "count_simple": [], "search_persistent": [], "search_simple": [], "box_count": [], "box_search": []}
                    ref = None
                    for rep in range(args.reps + 1):
                        for kernel in ("persistent", "simple"):
                            simple = kernel == "simple"
                            t, counts = pq.timed(torch, stream, lambda: ctx.tri_count(rec, simple=simple))
                            if rep:
                                ms["count_" + kernel].append(t)
                            t, res = pq.timed(torch, stream, lambda: ctx.tri_search(rec, capacity=cap, simple=simple))
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
                    ctx.tri_count(rec, stats=True)
                    st = ctx.stats()
                    med = {k: statistics.median(x) for k, x in ms.items()}
                    key = "%s_%d" % (sname, target)
                    ours = ("count_persistent", "count_simple", "search_persistent", "search_simple")
                    out[key] = {"caller_triangles": n, "size": size, "size_in_extents": round(size / extent, 6), "entries": total,
                                "entries_per_triangle": round(total / n, 3),
                                "ms": {k: round(med[k], 4) for k in ours},
                                "mtriangles_per_s": {k: round(n / (med[k] * 1e3), 1) for k in ours},
                                "mentries_per_s": {k: round(total / (med[k] * 1e3), 1) for k in ("search_persistent", "search_simple")},
                                "persistent_over_simple": {w: round(med[w + "_simple"] / med[w + "_persistent"], 3) for w in ("count", "search")},
                                "search_over_two_counts": {k: round(med["search_" + k] / (2 * med["count_" + k]), 3) for k in ("persistent", "simple")},
                                "box_yardstick": {"entries": box_total, "entries_per_box": round(box_total / n, 3),
                                                  "ms": {k: round(med["box_" + k], 4) for k in ("count", "search")},
                                                  "tri_over_box": {k: round(med[k + "_persistent"] / med["box_" + k], 3) for k in ("count", "search")}},
                                "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                                "stats": st,
                                "node_records_per_triangle": round(st["nodes_examined"] / n, 2),
                                "triangles_per_triangle": round(st["tris_tested"] / n, 2)}
                    print(name, "accel", accel, key, json.dumps({k: out[key][k] for k in ("entries_per_triangle", "mtriangles_per_s", "persistent_over_simple", "search_over_two_counts", "box_yardstick")}),
                          "drops", st["stack_drops"], "max_stack", st["max_stack"], flush=True)
                    save()
            ctx.close()
    result["complete"] = True
    save()
    print(json.dumps({n: {s: v["mtriangles_per_s"]["search_persistent"] for s, v in c["sets"].items()} for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
