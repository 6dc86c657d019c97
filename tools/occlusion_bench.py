#!/usr/bin/env python3
"""Throughput of the batched ambient-occlusion queries (include/mi355pt.h pt_occlusion) against what a caller had
to do before them, in one process, variants alternating, on C2 (dragon-class, 871,414 triangles, camera (0,0,2.5)) and C4 (sponza-class
interior, 262,144 triangles, camera inside), each with the reference's tree (accel 0) and the PLOC tree (accel 2).

Surfels: the hits of the 1920x1080 camera rays (pt_camera_rays -> pt_trace_rays -> pt_hit_surfels), misses dropped; all in device memory.
Per scene, tree, samples per surfel S in (16, 64) and r_max in (+inf, 0.25), four variants:
  F  pt_occlusion                                  the persistent kernel: rays built in registers, counted per surfel
  S  pt_occlusion(PT_OCCLUSION_SIMPLE_KERNEL)      one sample ray per thread
  C  the composition: pt_occlusion_rays + pt_trace_rays(PT_TRACE_ANY_HIT) + a torch count of the misses per surfel
  T  the pt_trace_rays leg of C alone, on the same ray records (the any-hit kernel as it was before this query existed)
Per variant: the median over --reps runs (after one warm-up) by events on the context's stream, in Mrays/s (rays = surfels * S), and the
ratios F/C, F/S, F/T of those rates.  F, S and C must give the same counts; the tool stops if they do not.

PB_BASE=1 in the environment runs the library of an earlier commit instead (tools/ab/README); the JSON records "build": "base" | "tree".

    python tools/occlusion_bench.py [--reps 5] [--out profiles/occlusion_ab.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")

W, H, SCENE_SEED = 1920, 1080, 20260109
CONFIGS = {
    "C2": dict(kind=0, n=871414, cam=(0, 0, 2.5), quat=(0, 0, 0, 1)),
    "C4": dict(kind=1, n=262144, cam=(0.55, -0.05, 0.05), quat=(0.0, 0.6630, 0.0, 0.7486)),
}
ACCELS = (0, 2)
SAMPLES = (16, 64)
R_MAX = (float("inf"), 0.25)
VARIANTS = ("F", "S", "C", "T")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    import torch
    # PB_BASE=1: the library of an earlier commit (tools/ab/raytracer_base, built by tools/ab/README) for an A/B within one session
    base = bool(os.environ.get("PB_BASE"))
    if base:
        sys.path.insert(0, os.path.join(ROOT, "tools", "ab"))
    rt = importlib.import_module("raytracer_base" if base else "raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/occlusion_bench.py", "build": "base" if base else "tree", "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "GPU_MAX_HW_QUEUES": os.environ["GPU_MAX_HW_QUEUES"], "resolution": [W, H], "rows": []}
    for name in args.configs.split(","):
        c = CONFIGS[name]
        tris = rt.procedural_scene(c["kind"], c["n"], SCENE_SEED)
        for accel in ACCELS:
            ctx = rt.Context(0)
            ctx.set_triangles(tris); ctx.build_bvh(accel)
            ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
            cam_rays = ctx.camera_rays(ctx.make_params(W, H, c["cam"], c["quat"]))
            cam_hits = ctx.trace_rays(cam_rays)
            for r_max in R_MAX:
                surfels = ctx.hit_surfels(cam_rays, cam_hits, r_max)
                surfels = surfels[surfels[:, 3] > 0].contiguous()        # the hits only
                n = surfels.shape[0]
                for S in SAMPLES:
                    kw = dict(seed=1, bias=1e-4)
                    rays = ctx.occlusion_rays(surfels, S, **kw)          # T's input (C writes its own every time)

                    def run(v):
                        if v == "F":
                            return ctx.occlusion(surfels, S, **kw)[1].view(torch.int32)
                        if v == "S":
                            return ctx.occlusion(surfels, S, simple=True, **kw)[1].view(torch.int32)
                        if v == "C":
                            r = ctx.occlusion_rays(surfels, S, **kw)
                            prim = ctx.trace_rays(r, any_hit=True)[1]
                            return (prim.view(torch.int32) == -1).reshape(n, S).sum(dim=1, dtype=torch.int32)
                        return ctx.trace_rays(rays, any_hit=True)[1]

                    ms = {v: [] for v in VARIANTS}
                    counts = {}
                    for rep in range(args.reps + 1):
                        for v in VARIANTS:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(stream)
                            res = run(v)
                            e1.record(stream)
                            e1.synchronize()
                            if rep:
                                ms[v].append(e0.elapsed_time(e1))
                            elif v != "T":
                                counts[v] = res.clone()
                            del res
                    assert torch.equal(counts["F"], counts["C"]) and torch.equal(counts["F"], counts["S"]), "the variants disagree"
                    med = {v: statistics.median(x) for v, x in ms.items()}
                    mr = {v: n * S / (med[v] * 1e3) for v in VARIANTS}
                    row = {"config": name, "accel": accel, "samples": S, "r_max": "inf" if r_max == float("inf") else r_max,
                           "surfels": n, "rays": n * S, "mean_visibility": round(float(counts["F"].double().mean()) / S, 4),
                           "ms": {v: round(med[v], 4) for v in VARIANTS},
                           "mrays_per_s": {v: round(mr[v], 1) for v in VARIANTS},
                           "F_over_C": round(mr["F"] / mr["C"], 3), "F_over_S": round(mr["F"] / mr["S"], 3), "F_over_T": round(mr["F"] / mr["T"], 3),
                           "ms_all": {v: [round(x, 4) for x in ms[v]] for v in VARIANTS}}
                    result["rows"].append(row)
                    print(json.dumps({k: row[k] for k in ("config", "accel", "samples", "r_max", "rays", "mrays_per_s", "F_over_C", "F_over_S", "F_over_T")}), flush=True)
                    del rays, counts
                    torch.cuda.empty_cache()
            ctx.close()
    result["F_at_least_C_on_every_row"] = all(r["F_over_C"] >= 1.0 for r in result["rows"])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"rows": len(result["rows"]), "min_F_over_C": min(r["F_over_C"] for r in result["rows"]),
                      "F_at_least_C_on_every_row": result["F_at_least_C_on_every_row"]}))


if __name__ == "__main__":
    main()
