#!/usr/bin/env python3
"""Throughput of the hit lists (include/mi355pt.h pt_list_hits): the persistent kernel against the simple
one-ray-per-thread kernel, unsorted against sorted, in one process, variants alternating, on C2 (dragon-class, 871,414 triangles, camera
(0,0,2.5)) and C4 (sponza-class interior, 262,144 triangles, camera inside).

Ray sets: the camera rays (coherent) and the diffuse bounce rays (incoherent) of tools/rayquery_bench.py, in device memory (torch
tensors, zero-copy).  Per set and variant: the median over --reps launches (after one warm-up) of the time by events on the context's
stream of pt_list_hits with a capacity that holds every entry (no host wait): the count walk, the scan, the fill walk and, sorted, the
sort.  Next to it the count alone (pt_count_hits), so that list_over_two_counts = ms(list) / (2 x ms(count)) says what the scan, the
16-byte stores and the sort add to walking twice.  Reported in Mrays/s and Mentries/s, with the distribution of list lengths (mean,
maximum, the share of lists above PT_HL_LANE_MAX = 16) and stack_drops / max_stack from one PT_HITS_STATS pass.  The variants must give
the same sorted lists; the tool stops if they do not.  There is no gate: the query has no predecessor.

PB_BASE=1 in the environment runs the library of an earlier commit instead (tools/ab/README); the JSON records "build": "base" | "tree".

    python tools/hitlist_bench.py [--reps 5] [--out profiles/hitlist_ab.json]      (--out defaults to that file)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")       # the package's own default; recorded in the output

import rayquery_bench as rq  # noqa: E402  (the configurations and the ray sets)

VARIANTS = {"persistent": dict(simple=False, sort=False), "simple": dict(simple=True, sort=False),
            "persistent_sorted": dict(simple=False, sort=True), "simple_sorted": dict(simple=True, sort=True)}


def timed(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    res = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hitlist_ab.json"))
    ap.add_argument("--configs", default=",".join(rq.CONFIGS))
    args = ap.parse_args()
    import torch
    # PB_BASE=1: the library of an earlier commit (tools/ab/raytracer_base, built by tools/ab/README) for an A/B within one session
    base = bool(os.environ.get("PB_BASE"))
    if base:
        sys.path.insert(0, os.path.join(ROOT, "tools", "ab"))
    rt = importlib.import_module("raytracer_base" if base else "raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/hitlist_bench.py", "build": "base" if base else "tree", "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "configs": {}}
    for name in args.configs.split(","):
        c = rq.CONFIGS[name]
        rng = np.random.default_rng(rq.RNG_SEED)
        tris = rt.procedural_scene(c["kind"], c["n"], rq.SCENE_SEED)
        ctx = rt.Context(0)
        ctx.set_triangles(tris); ctx.build_bvh()
        ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
        diffuse, _ = rq.secondary_sets(rt, ctx, tris, c["cam"], c["quat"], rng)
        sets = {"a_camera": ctx.camera_rays(ctx.make_params(rq.W, rq.H, c["cam"], c["quat"])), "b_diffuse": torch.from_numpy(diffuse).cuda()}
        out = {}
        for sname, rays in sets.items():
            n = rays.shape[0]
            counts = ctx.count_hits(rays).view(torch.int32).to(torch.int64)
            total = int(counts.sum().item())
            cap = total + 64
            ms = {k: [] for k in list(VARIANTS) + ["count_persistent", "count_simple"]}
            ref = None
            for rep in range(args.reps + 1):
                for k, kw in VARIANTS.items():
                    if not kw["sort"]:
                        t, cnt = timed(torch, stream, lambda: ctx.count_hits(rays, simple=kw["simple"]))
                        if rep:
                            ms["count_" + k].append(t)
                    t, res = timed(torch, stream, lambda: ctx.list_hits(rays, capacity=cap, **kw))
                    if rep:
                        ms[k].append(t)
                    assert int(res[0][-1]) == total and torch.equal(torch.diff(res[0]), counts), "counts and offsets disagree"
                    if kw["sort"]:
                        got = [x.view(torch.int32)[:total] for x in res[1:]]
                        if ref is None:
                            ref = got
                        else:
                            assert all(torch.equal(a, b) for a, b in zip(ref, got)), "the kernels disagree"
            ctx.list_hits(rays, capacity=cap, stats=True)
            st = ctx.stats()
            med = {k: statistics.median(x) for k, x in ms.items()}
            out[sname] = {"rays": n, "entries": total, "entries_per_ray": round(total / n, 3), "longest_list": int(counts.max().item()),
                          "lists_above_lane_max": int((counts > 16).sum().item()),
                          "ms": {k: round(x, 4) for k, x in med.items()},
                          "mrays_per_s": {k: round(n / (x * 1e3), 1) for k, x in med.items()},
                          "mentries_per_s": {k: round(total / (med[k] * 1e3), 1) for k in VARIANTS},
                          "persistent_over_simple": {w: round(med["simple" + w] / med["persistent" + w], 3) for w in ("", "_sorted")},
                          "sorted_over_unsorted": {k: round(med[k + "_sorted"] / med[k], 3) for k in ("persistent", "simple")},
                          "list_over_two_counts": {k: round(med[k] / (2 * med["count_" + k]), 3) for k in ("persistent", "simple")},
                          "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                          "stats": st}
            print(name, sname, json.dumps({k: out[sname][k] for k in ("entries_per_ray", "longest_list", "mrays_per_s", "sorted_over_unsorted", "list_over_two_counts")}),
                  "drops", st["stack_drops"], "max_stack", st["max_stack"], flush=True)
        result["configs"][name] = {"triangles": c["n"], "sets": out}
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({n: {s: v["mrays_per_s"]["persistent_sorted"] for s, v in c["sets"].items()} for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
