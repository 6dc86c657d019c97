#!/usr/bin/env python3
"""Throughput of the box-overlap queries (include/mi355pt.h pt_box_count / pt_box_search): the persistent kernel
against the simple one-box-per-thread kernel, and the search (count walk + scan + fill walk) against two calls of the count, in one
process, kernels alternating, on C2 (dragon-class, 871,414 triangles) and C4 (sponza-class interior, 262,144 triangles), each at build
level 0 and 2.

Box sets: cubes around the three point sets of tools/pointquery_bench.py (surface, box, far), the first 262,144 points of each, in device
memory (torch tensors, zero-copy).  Per set three sizes, one common half-extent per set, found by bisection on the first 16,384 boxes so
that the mean list length is about 1, 8 and 64 entries per box; the lengths actually obtained are recorded.
Per set, size and kernel: the median over --reps launches (after one warm-up) of the launch time by events on the context's stream, of
  count   pt_box_count
  search  pt_box_search with a capacity that holds every entry (no host wait)
in Mboxes/s and, for the search, Mentries/s.  search_over_two_counts = ms(search) / (2 x ms(count)): the fill walk repeats the count
walk, so 1.0 means that the scan and the 16-byte stores cost nothing.  Per set and size: node records and triangles per box, stack_drops
and max_stack from one PT_BOX_STATS pass.  There is no gate: the query has no predecessor.

    python tools/box_bench.py [--reps 5] [--configs C2,C4] [--out profiles/box_ab.json]      (--out defaults to that file)
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

N_BOXES, N_CALIBRATE = 262144, 16384
TARGETS = (1, 8, 64)


def cubes(torch, centres, half):
    """(n, 8) PtBox records on the device: centres +- half"""
    z = torch.zeros((centres.shape[0], 1), dtype=torch.float32, device=centres.device)
    return torch.cat([centres - half, z, centres + half, z], dim=1).contiguous()


def half_for(ctx, torch, centres, target, extent):
    """The common half-extent at which the first N_CALIBRATE cubes have `target` entries on average (bisection in log h)."""
    sub = centres[:N_CALIBRATE]
    lo, hi = 1e-5 * extent, 16.0 * extent
    for _ in range(40):
        h = float(np.sqrt(lo * hi))
        mean = float(ctx.box_count(cubes(torch, sub, h)).view(torch.int32).sum(dtype=torch.int64).item()) / N_CALIBRATE
        if mean < target:
            lo = h
        else:
            hi = h
    return float(np.float32(hi))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default=",".join(pq.CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_ab.json"))
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/box_bench.py", "reps": args.reps, "device": torch.cuda.get_device_name(0), "boxes": N_BOXES,
              "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "configs": {}}
    for name in args.configs.split(","):
        c = pq.CONFIGS[name]
        tris = rt.procedural_scene(c["kind"], c["n"], pq.SCENE_SEED)
        v = tris.reshape(-1, 3)
        extent = float((v.max(0) - v.min(0)).max())
        sets = {k: torch.from_numpy(np.ascontiguousarray(p[:N_BOXES])).cuda() for k, p in pq.point_sets(tris, np.random.default_rng(pq.RNG_SEED)).items()}
        for accel in pq.ACCELS:
            ctx = rt.Context(0)
            ctx.set_triangles(tris); ctx.build_bvh(accel)
            ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
            out = {}
            for sname, centres in sets.items():
                n = centres.shape[0]
                for target in TARGETS:
                    half = half_for(ctx, torch, centres, target, extent)
                    boxes = cubes(torch, centres, half)
                    total = int(ctx.box_count(boxes).view(torch.int32).sum(dtype=torch.int64).item())
                    cap = total + 64
                    ms = {"count_persistent": [], "count_simple": [], "search_persistent": [], "search_simple": []}
                    ref = None
                    for rep in range(args.reps + 1):
                        for kernel in ("persistent", "simple"):
                            simple = kernel == "simple"
                            t, counts = pq.timed(torch, stream, lambda: ctx.box_count(boxes, simple=simple))
                            if rep:
                                ms["count_" + kernel].append(t)
                            t, res = pq.timed(torch, stream, lambda: ctx.box_search(boxes, capacity=cap, simple=simple))
                            if rep:
                                ms["search_" + kernel].append(t)
                            got = [res[0]] + [x.view(torch.int32)[:total] for x in res[1:]]
                            if ref is None:
                                ref = got
                                assert int(res[0][-1]) == total and torch.equal(torch.diff(res[0]), counts.view(torch.int32).to(torch.int64)), "counts and offsets disagree"
                            else:
                                assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the kernels disagree"
                    ctx.box_count(boxes, stats=True)
                    st = ctx.stats()
                    med = {k: statistics.median(x) for k, x in ms.items()}
                    key = "%s_%d" % (sname, target)
                    out[key] = {"boxes": n, "half_extent": half, "half_extent_in_extents": round(half / extent, 6), "entries": total,
                                "entries_per_box": round(total / n, 3),
                                "ms": {k: round(x, 4) for k, x in med.items()},
                                "mboxes_per_s": {k: round(n / (x * 1e3), 1) for k, x in med.items()},
                                "mentries_per_s": {k: round(total / (med[k] * 1e3), 1) for k in ("search_persistent", "search_simple")},
                                "persistent_over_simple": {w: round(med[w + "_simple"] / med[w + "_persistent"], 3) for w in ("count", "search")},
                                "search_over_two_counts": {k: round(med["search_" + k] / (2 * med["count_" + k]), 3) for k in ("persistent", "simple")},
                                "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                                "stats": st,
                                "node_records_per_box": round(st["nodes_examined"] / n, 2),
                                "triangles_per_box": round(st["tris_tested"] / n, 2)}
                    print(name, "accel", accel, key, json.dumps({k: out[key][k] for k in ("entries_per_box", "mboxes_per_s", "persistent_over_simple", "search_over_two_counts")}),
                          "drops", st["stack_drops"], "max_stack", st["max_stack"], flush=True)
            result["configs"]["%s_accel%d" % (name, accel)] = {"triangles": c["n"], "accel": accel, "extent": extent, "sets": out}
            ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({n: {s: v["mboxes_per_s"]["search_persistent"] for s, v in c["sets"].items()} for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
