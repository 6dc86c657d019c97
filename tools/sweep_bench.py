#!/usr/bin/env python3
"""Throughput of the sphere-cast queries (include/mi355pt.h pt_sweep_spheres): the persistent kernel against the
simple one-sweep-per-thread kernel, in one process, kernels alternating, on C2 (dragon-class, 871,414 triangles, camera (0,0,2.5)) and
C4 (sponza-class interior, 262,144 triangles, camera inside), as tools/rayquery_bench.py does for the ray queries.

Sweep sets, all in device memory (torch tensors, zero-copy), each at the radii 0, 1 % and 5 % of the scene extent:
  (a) camera     -- the 1920x1080 camera rays of PT_MODE_REFERENCE (pt_camera_rays) as sweeps;
  (b) incoherent -- 2,073,600 sweeps from the hit points of jittered primaries (one per pixel), offset along the facing normal by the
                    radius + 1e-4 so that the sphere starts clear of the surface it leaves, cosine directions from a seeded numpy RNG.
Per set, radius and kernel: the median over --reps launches (after one warm-up) of the launch time by events on the context's stream, in
Msweeps/s.  Per set and radius: node records and triangles per item from one PT_SWEEP_STATS pass.  The JSON records GPU_MAX_HW_QUEUES.

    python tools/sweep_bench.py [--reps 3] [--out profiles/sweep_ab.json]
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

from rayquery_bench import CONFIGS, H, RNG_SEED, SCENE_SEED, W, jittered_primaries  # noqa: E402

RADII = (0.0, 0.01, 0.05)        # of the scene extent


def incoherent(rt, ctx, tris, cam, quat, rng, radius):
    """(n, 8) float32 PtSweep records leaving the surface the camera sees, in cosine-distributed directions."""
    O, D = jittered_primaries(rt, cam, quat, rng, 1)
    t, prim, _, _ = ctx.trace_rays(O, D)
    hit = np.flatnonzero(prim != rt.PRIM_NONE)
    pick = hit[rng.integers(0, hit.size, W * H)]
    T = tris.reshape(-1, 3, 3)[prim[pick]]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = D[pick]
    n = np.where((np.sum(n * d, 1) < 0)[:, None], n, -n).astype(np.float32)          # facing the incoming ray
    p = (O[pick] + d * t[pick][:, None] + n * np.float32(radius + 1e-4)).astype(np.float32)
    u1, u2 = rng.random(len(p), dtype=np.float32), rng.random(len(p), dtype=np.float32)
    r, phi = np.sqrt(u1), np.float32(2 * np.pi) * u2
    a = np.where(np.abs(n[:, :1]) > 0.9, np.float32([[0, 1, 0]]), np.float32([[1, 0, 0]]))
    tt = np.cross(a, n); tt /= np.linalg.norm(tt, axis=1, keepdims=True); bb = np.cross(n, tt)
    dd = (tt * (r * np.cos(phi))[:, None] + bb * (r * np.sin(phi))[:, None] + n * np.sqrt(1 - u1)[:, None]).astype(np.float32)
    return rt.pack_sweeps(p, dd, radius)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/sweep_bench.py", "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "radii_of_extent": list(RADII), "configs": {}}
    for name, c in CONFIGS.items():
        tris = rt.procedural_scene(c["kind"], c["n"], SCENE_SEED)
        v = tris.reshape(-1, 3)
        extent = float((v.max(0) - v.min(0)).max())
        ctx = rt.Context(0)
        ctx.set_triangles(tris); ctx.build_bvh()
        ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
        camera = ctx.camera_rays(ctx.make_params(W, H, c["cam"], c["quat"]))
        out = {}
        for frac in RADII:
            radius = frac * extent
            cam_sweeps = camera.clone(); cam_sweeps[:, 7] = radius
            sets = {"a_camera": cam_sweeps,
                    "b_incoherent": torch.from_numpy(incoherent(rt, ctx, tris, c["cam"], c["quat"], np.random.default_rng(RNG_SEED), radius)).cuda()}
            for sname, sweeps in sets.items():
                n = sweeps.shape[0]
                ms = {"persistent": [], "simple": []}
                for rep in range(args.reps + 1):
                    for kernel in ("persistent", "simple"):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        res = ctx.sweep_spheres(sweeps, simple=kernel == "simple")
                        e1.record(stream)
                        e1.synchronize()
                        if rep:
                            ms[kernel].append(e0.elapsed_time(e1))
                        if kernel == "persistent":
                            ref = torch.stack([x.view(torch.int32) for x in res])
                        else:
                            assert torch.equal(ref, torch.stack([x.view(torch.int32) for x in res])), "the kernels disagree"
                hits = int((ref[1] != -1).sum())
                at_start = int((ref[0] == 0).sum())
                ctx.sweep_spheres(sweeps, stats=True)
                st = ctx.stats()
                med = {k: statistics.median(v) for k, v in ms.items()}
                key = "%s_r%g" % (sname, frac)
                out[key] = {"sweeps": n, "radius": radius, "hits": hits, "t_zero": at_start,
                            "ms": {k: round(v, 4) for k, v in med.items()},
                            "msweeps_per_s": {k: round(n / (v * 1e3), 1) for k, v in med.items()},
                            "persistent_over_simple": round(med["simple"] / med["persistent"], 3),
                            "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                            "stats": st,
                            "node_records_per_item": round(st["nodes_examined"] / n, 2),
                            "triangles_per_item": round(st["tris_tested"] / n, 2)}
                print(name, key, json.dumps({k: out[key][k] for k in ("sweeps", "msweeps_per_s", "persistent_over_simple", "node_records_per_item", "triangles_per_item")}), flush=True)
        result["configs"][name] = {"triangles": c["n"], "extent": extent, "camera": [c["cam"], c["quat"]], "sets": out}
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({n: {s: v["msweeps_per_s"] for s, v in c["sets"].items()} for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
