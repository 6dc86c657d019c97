#!/usr/bin/env python3
"""Throughput of the batched closest-point queries (include/mi355pt.h pt_closest_points): the persistent kernel
against the simple one-point-per-thread kernel, in one process, kernels alternating, on C2 (dragon-class, 871,414 triangles) and C4
(sponza-class interior, 262,144 triangles), each at build level 0 and 2.

Point sets, all in device memory (torch tensors, zero-copy), 2,073,600 points each, r_max = +inf:
  (a) surface -- within 0.01 of the surface: a random triangle, a random point on it, an offset of up to 0.01 along its normal;
  (b) box     -- uniform in 1.5x the scene box;
  (c) far     -- 4 to 10 scene extents (the longest edge of the scene box) away from the scene's centre, in a random direction.
Per set and kernel: the median over --reps launches (after one warm-up) of the launch time by events on the context's stream, in
Mpoints/s.  Per set: node records and triangles per point from one PT_CLOSEST_STATS pass.  For scale: the brute-force kernel on a
20,000-point subset of (b).

    python tools/pointquery_bench.py [--reps 5] [--out profiles/pointquery_ab.json]
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
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")       # the package's own default; recorded in the output

SCENE_SEED, RNG_SEED = 20260109, 7
N_POINTS, N_BRUTE = 2073600, 20000
CONFIGS = {"C2": dict(kind=0, n=871414), "C4": dict(kind=1, n=262144)}
ACCELS = (0, 2)


def point_sets(tris, rng):
    T = tris.reshape(-1, 3, 3)
    lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
    mid, half = (lo + hi) * np.float32(0.5), (hi - lo) * np.float32(0.5)
    extent = float((hi - lo).max())
    pick = rng.integers(0, len(T), N_POINTS)
    b = rng.random((N_POINTS, 2), dtype=np.float32); b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    e1, e2 = T[pick, 1] - T[pick, 0], T[pick, 2] - T[pick, 0]
    n = np.cross(e1, e2); n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    surface = T[pick, 0] + b[:, :1] * e1 + b[:, 1:] * e2 + n * rng.uniform(-0.01, 0.01, (N_POINTS, 1)).astype(np.float32)
    box = mid + (rng.random((N_POINTS, 3), dtype=np.float32) * 2 - 1) * half * np.float32(1.5)
    d = rng.normal(size=(N_POINTS, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = mid + d * (rng.uniform(4, 10, (N_POINTS, 1)) * extent).astype(np.float32)
    return {"a_surface": surface.astype(np.float32), "b_box": box.astype(np.float32), "c_far": far.astype(np.float32)}


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/pointquery_bench.py", "reps": args.reps, "device": torch.cuda.get_device_name(0), "points": N_POINTS,
              "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "configs": {}}
    for name, c in CONFIGS.items():
        tris = rt.procedural_scene(c["kind"], c["n"], SCENE_SEED)
        sets = {k: torch.from_numpy(rt.pack_points(v)).cuda() for k, v in point_sets(tris, np.random.default_rng(RNG_SEED)).items()}
        for accel in ACCELS:
            ctx = rt.Context(0)
            ctx.set_triangles(tris); ctx.build_bvh(accel)
            ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
            out = {}
            for sname, pts in sets.items():
                n = pts.shape[0]
                ms = {"persistent": [], "simple": []}
                for rep in range(args.reps + 1):
                    for kernel in ("persistent", "simple"):
                        t, res = timed(torch, stream, lambda: ctx.closest_points(pts, simple=kernel == "simple"))
                        if rep:
                            ms[kernel].append(t)
                        if kernel == "persistent":
                            ref = torch.stack([x.view(torch.int32) for x in res])
                        else:
                            assert torch.equal(ref, torch.stack([x.view(torch.int32) for x in res])), "the kernels disagree"
                ctx.closest_points(pts, stats=True)
                st = ctx.stats()
                med = {k: statistics.median(v) for k, v in ms.items()}
                out[sname] = {"points": n, "ms": {k: round(v, 4) for k, v in med.items()},
                              "mpoints_per_s": {k: round(n / (v * 1e3), 1) for k, v in med.items()},
                              "persistent_over_simple": round(med["simple"] / med["persistent"], 3),
                              "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                              "stats": st,
                              "node_records_per_point": round(st["nodes_examined"] / n, 2),
                              "triangles_per_point": round(st["tris_tested"] / n, 2)}
                print(name, "accel", accel, sname, json.dumps({k: out[sname][k] for k in ("mpoints_per_s", "persistent_over_simple", "node_records_per_point", "triangles_per_point")}), flush=True)
            sub = sets["b_box"][:N_BRUTE].contiguous()
            bms = []
            for rep in range(args.reps + 1):
                t, res = timed(torch, stream, lambda: ctx.closest_points(sub, brute_force=True))
                if rep:
                    bms.append(t)
            tree = ctx.closest_points(sub)
            assert torch.equal(res[0].view(torch.int32), tree[0].view(torch.int32)), "tree and brute force disagree on dist"
            bmed = statistics.median(bms)
            brute = {"points": N_BRUTE, "ms": round(bmed, 3), "mpoints_per_s": round(N_BRUTE / (bmed * 1e3), 3),
                     "point_triangle_tests_per_s": round(N_BRUTE * c["n"] / (bmed * 1e-3), 0)}
            print(name, "accel", accel, "brute", json.dumps(brute), flush=True)
            result["configs"]["%s_accel%d" % (name, accel)] = {"triangles": c["n"], "accel": accel, "sets": out, "brute_force_on_b": brute}
            ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({n: {s: v["mpoints_per_s"] for s, v in c["sets"].items()} for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
