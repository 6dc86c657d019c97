#!/usr/bin/env python3
"""Throughput of the crossing-count and containment queries (include/mi355pt.h pt_count_hits, pt_contains), in one
process, variants alternating, on C2 (dragon-class, 871,414 triangles, camera (0,0,2.5)) and C4 (sponza-class interior, 262,144
triangles, camera inside).

count_hits: the persistent kernel against the simple one-ray-per-thread kernel on the ray sets of tools/rayquery_bench.py (camera,
diffuse, shadow), all in device memory; next to them the closest-hit / any-hit query of the same rays (pt_trace_rays), which stops at the
first surface where the count goes on to the last.
contains: --points points uniform in the scene's box, samples per point S in (1, 3, 7), three variants:
  F  pt_contains                                   the persistent kernel: rays built in registers, parities counted per point
  S  pt_contains(PT_CONTAIN_SIMPLE_KERNEL)         one sample ray per thread
  C  the composition: pt_occlusion_rays + pt_count_hits + a torch parity count per point
Per variant: the median over --reps runs (after one warm-up) by events on the context's stream, in Mrays/s.  The variants must give the
same results; the tool stops if they do not.  There is no gate: the queries have no predecessor to be measured against.

PB_BASE=1 in the environment runs the library of an earlier commit instead (tools/ab/README); the JSON records "build": "base" | "tree".

    python tools/crossings_bench.py [--reps 5] [--points 2000000] [--out profiles/crossings_ab.json]
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
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")

import rayquery_bench as rq  # noqa: E402  (the configurations and the ray sets)

SAMPLES = (1, 3, 7)


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
    ap.add_argument("--points", type=int, default=2000000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default=",".join(rq.CONFIGS))
    args = ap.parse_args()
    import torch
    # PB_BASE=1: the library of an earlier commit (tools/ab/raytracer_base, built by tools/ab/README) for an A/B within one session
    base = bool(os.environ.get("PB_BASE"))
    if base:
        sys.path.insert(0, os.path.join(ROOT, "tools", "ab"))
    rt = importlib.import_module("raytracer_base" if base else "raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/crossings_bench.py", "build": "base" if base else "tree", "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "GPU_MAX_HW_QUEUES": os.environ["GPU_MAX_HW_QUEUES"], "configs": {}}
    for name in args.configs.split(","):
        c = rq.CONFIGS[name]
        rng = np.random.default_rng(rq.RNG_SEED)
        tris = rt.procedural_scene(c["kind"], c["n"], rq.SCENE_SEED)
        ctx = rt.Context(0)
        ctx.set_triangles(tris); ctx.build_bvh()
        ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
        diffuse, shadow = rq.secondary_sets(rt, ctx, tris, c["cam"], c["quat"], rng)
        sets = {"a_camera": (ctx.camera_rays(ctx.make_params(rq.W, rq.H, c["cam"], c["quat"])), False),
                "b_diffuse": (torch.from_numpy(diffuse).cuda(), False),
                "c_shadow": (torch.from_numpy(shadow).cuda(), True)}
        count_rows = {}
        for sname, (rays, anyhit) in sets.items():
            n = rays.shape[0]
            variants = {"persistent": lambda: ctx.count_hits(rays), "simple": lambda: ctx.count_hits(rays, simple=True),
                        "trace_rays": lambda: ctx.trace_rays(rays, any_hit=anyhit)[1]}
            ms = {k: [] for k in variants}
            ref = None
            for rep in range(args.reps + 1):
                for k, fn in variants.items():
                    t, res = timed(torch, stream, fn)
                    if rep:
                        ms[k].append(t)
                    if k == "persistent":
                        ref = res.view(torch.int32).clone()
                    elif k == "simple":
                        assert torch.equal(ref, res.view(torch.int32)), "the kernels disagree"
                    else:
                        assert torch.equal(ref >= 1, res.view(torch.int32) != -1), "count >= 1 and the hit flag disagree"
                    del res
            ctx.count_hits(rays, stats=True)
            st = ctx.stats()
            med = {k: statistics.median(v) for k, v in ms.items()}
            count_rows[sname] = {"rays": n, "crossings": int(ref.sum()), "rays_crossing_something": int((ref >= 1).sum()), "max_count": int(ref.max()),
                                 "ms": {k: round(v, 4) for k, v in med.items()},
                                 "mrays_per_s": {k: round(n / (v * 1e3), 1) for k, v in med.items()},
                                 "persistent_over_simple": round(med["simple"] / med["persistent"], 3),
                                 "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                                 "stats": st, "node_records_per_ray": round(st["nodes_examined"] / n, 2)}
            print(name, sname, json.dumps({k: count_rows[sname][k] for k in ("rays", "mrays_per_s", "persistent_over_simple", "node_records_per_ray")}), flush=True)
        del sets, diffuse, shadow
        torch.cuda.empty_cache()
        v = tris.reshape(-1, 3)
        lo, hi = v.min(axis=0), v.max(axis=0)
        pts_np = np.full((args.points, 4), np.inf, np.float32)
        pts_np[:, :3] = lo + rng.random((args.points, 3), dtype=np.float32) * (hi - lo)
        pts = torch.from_numpy(pts_np).cuda()
        surfels = torch.zeros((args.points, 8), dtype=torch.float32, device="cuda")
        surfels[:, :4] = pts; surfels[:, 6] = 1.0
        contain_rows = []
        for S in SAMPLES:
            kw = dict(seed=1, index_base=0)

            def composition():
                r = ctx.occlusion_rays(surfels, S, bias=0.0, **kw)
                odd = (ctx.count_hits(r).view(torch.int32) & 1).reshape(args.points, S).sum(dim=1, dtype=torch.int32)
                return odd
            variants = {"F": lambda: ctx.contains(pts, samples=S, **kw)[1].view(torch.int32),
                        "S": lambda: ctx.contains(pts, samples=S, simple=True, **kw)[1].view(torch.int32), "C": composition}
            ms = {k: [] for k in variants}
            odd = {}
            for rep in range(args.reps + 1):
                for k, fn in variants.items():
                    t, res = timed(torch, stream, fn)
                    if rep:
                        ms[k].append(t)
                    else:
                        odd[k] = res.clone()
                    del res
            assert torch.equal(odd["F"], odd["C"]) and torch.equal(odd["F"], odd["S"]), "the variants disagree"
            med = {k: statistics.median(x) for k, x in ms.items()}
            mr = {k: args.points * S / (med[k] * 1e3) for k in variants}
            row = {"samples": S, "points": args.points, "rays": args.points * S, "inside_share": round(float((2 * odd["F"] > S).double().mean()), 4),
                   "unanimous_share": round(float(((odd["F"] == 0) | (odd["F"] == S)).double().mean()), 4),
                   "ms": {k: round(med[k], 4) for k in variants}, "mrays_per_s": {k: round(mr[k], 1) for k in variants},
                   "F_over_C": round(mr["F"] / mr["C"], 3), "F_over_S": round(mr["F"] / mr["S"], 3),
                   "ms_all": {k: [round(x, 4) for x in ms[k]] for k in variants}}
            contain_rows.append(row)
            print(name, "contains", json.dumps({k: row[k] for k in ("samples", "rays", "mrays_per_s", "F_over_C", "F_over_S", "inside_share")}), flush=True)
            del odd
            torch.cuda.empty_cache()
        result["configs"][name] = {"triangles": c["n"], "camera": [c["cam"], c["quat"]], "count_hits": count_rows, "contains": contain_rows}
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({n: {"count_hits": {s: v["mrays_per_s"] for s, v in c["count_hits"].items()},
                          "contains": {r["samples"]: r["mrays_per_s"] for r in c["contains"]}} for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
