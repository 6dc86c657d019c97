#!/usr/bin/env python3
"""Throughput of the batched ray queries (include/mi355pt.h pt_trace_rays): the persistent kernel against the
simple one-ray-per-thread kernel, in one process, kernels alternating, on C2 (dragon-class, 871,414 triangles, camera (0,0,2.5)) and
C4 (sponza-class interior, 262,144 triangles, camera inside).

Ray sets, all in device memory (torch tensors, zero-copy):
  (a) camera  -- the 1920x1080 camera rays of PT_MODE_REFERENCE (pt_camera_rays), closest hit;
  (b) diffuse -- 8,294,400 incoherent rays: hit points of jittered primaries (4 per pixel), offset 1e-4 along the facing normal, cosine
                 directions from a seeded numpy RNG, closest hit;
  (c) shadow  -- from the same points toward light_dir() = normalize(1, 1.5, 1), any hit.
Per set and kernel: the median over --reps launches (after one warm-up) of the launch time by events on the context's stream, in Mrays/s.
Per set: node records examined in one PT_TRACE_STATS pass, and those per second at the persistent kernel's time -- next to the
megakernel's rate on C2 (BENCH_r06: about 410 M records per 0.69 ms frame).

PB_BASE=1 in the environment runs the library of an earlier commit instead (tools/ab/README); the JSON records "build": "base" | "tree".

    python tools/rayquery_bench.py [--reps 5] [--out profiles/rayquery_ab.json]
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
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")

W, H, SCENE_SEED, RNG_SEED = 1920, 1080, 20260109, 7
N_DIFFUSE = 8294400
CONFIGS = {
    "C2": dict(kind=0, n=871414, cam=(0, 0, 2.5), quat=(0, 0, 0, 1)),
    "C4": dict(kind=1, n=262144, cam=(0.55, -0.05, 0.05), quat=(0.0, 0.6630, 0.0, 0.7486)),
}
MEGAKERNEL_C2 = {"node_records_per_frame": 410e6, "ms_per_frame": 0.69, "source": "BENCH_r06.json"}


def rotate(v, q):
    u, s = np.asarray(q[:3], np.float32), np.float32(q[3])
    uv = np.cross(u, v); uuv = np.cross(u, uv)
    return (v + 2 * (s * uv + uuv)).astype(np.float32)


def jittered_primaries(rt, cam, quat, rng, spp):
    focal, aspect = rt.focal_aspect(W, H)
    py, px = np.divmod(np.repeat(np.arange(W * H), spp), W)
    fx = (px + rng.random(px.size, dtype=np.float32)) / np.float32(W) * 2 - 1
    fy = (py + rng.random(py.size, dtype=np.float32)) / np.float32(H) * 2 - 1
    d = np.stack([fx * np.float32(aspect), fy, np.full(fx.size, -focal, np.float32)], 1).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(np.asarray(cam, np.float32), d.shape).copy(), rotate(d, quat)


def secondary_sets(rt, ctx, tris, cam, quat, rng):
    """(diffuse rays, shadow rays) as (n, 8) float32 PtRay records."""
    O, D = jittered_primaries(rt, cam, quat, rng, 4)
    t, prim, _, _ = ctx.trace_rays(O, D)
    hit = np.flatnonzero(prim != rt.PRIM_NONE)
    pick = hit[rng.integers(0, hit.size, N_DIFFUSE)]
    T = tris.reshape(-1, 3, 3)[prim[pick]]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = D[pick]
    n = np.where((np.sum(n * d, 1) < 0)[:, None], n, -n).astype(np.float32)          # facing the incoming ray
    p = (O[pick] + d * t[pick][:, None] + n * np.float32(1e-4)).astype(np.float32)
    u1, u2 = rng.random(N_DIFFUSE, dtype=np.float32), rng.random(N_DIFFUSE, dtype=np.float32)
    r, phi = np.sqrt(u1), np.float32(2 * np.pi) * u2
    a = np.where(np.abs(n[:, :1]) > 0.9, np.float32([[0, 1, 0]]), np.float32([[1, 0, 0]]))
    tt = np.cross(a, n); tt /= np.linalg.norm(tt, axis=1, keepdims=True); bb = np.cross(n, tt)
    dd = (tt * (r * np.cos(phi))[:, None] + bb * (r * np.sin(phi))[:, None] + n * np.sqrt(1 - u1)[:, None]).astype(np.float32)
    L = np.float32([1, 1.5, 1]); L /= np.linalg.norm(L)
    return rt.pack_rays(p, dd), rt.pack_rays(p, np.broadcast_to(L, p.shape))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    # PB_BASE=1: the library of an earlier commit (tools/ab/raytracer_base, built by tools/ab/README) for an A/B within one session
    base = bool(os.environ.get("PB_BASE"))
    if base:
        sys.path.insert(0, os.path.join(ROOT, "tools", "ab"))
    rt = importlib.import_module("raytracer_base" if base else "raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/rayquery_bench.py", "build": "base" if base else "tree", "reps": args.reps, "device": torch.cuda.get_device_name(0), "configs": {},
              "megakernel_c2_reference": dict(MEGAKERNEL_C2, node_records_per_s=MEGAKERNEL_C2["node_records_per_frame"] / (MEGAKERNEL_C2["ms_per_frame"] * 1e-3))}
    for name, c in CONFIGS.items():
        rng = np.random.default_rng(RNG_SEED)
        tris = rt.procedural_scene(c["kind"], c["n"], SCENE_SEED)
        ctx = rt.Context(0)
        ctx.set_triangles(tris); ctx.build_bvh()
        ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
        diffuse, shadow = secondary_sets(rt, ctx, tris, c["cam"], c["quat"], rng)
        sets = {"a_camera": (ctx.camera_rays(ctx.make_params(W, H, c["cam"], c["quat"])), False),
                "b_diffuse": (torch.from_numpy(diffuse).cuda(), False),
                "c_shadow_anyhit": (torch.from_numpy(shadow).cuda(), True)}
        out = {}
        for sname, (rays, anyhit) in sets.items():
            n = rays.shape[0]
            ms = {"persistent": [], "simple": []}
            for rep in range(args.reps + 1):
                for kernel in ("persistent", "simple"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    res = ctx.trace_rays(rays, any_hit=anyhit, simple=kernel == "simple")
                    e1.record(stream)
                    e1.synchronize()
                    if rep:
                        ms[kernel].append(e0.elapsed_time(e1))
                    if kernel == "persistent":
                        ref = torch.stack([x.view(torch.int32) for x in res])
                    else:
                        assert torch.equal(ref, torch.stack([x.view(torch.int32) for x in res])), "the kernels disagree"
            hits = int((ref[1] != -1).sum())
            ctx.trace_rays(rays, any_hit=anyhit, stats=True)
            st = ctx.stats()
            med = {k: statistics.median(v) for k, v in ms.items()}
            out[sname] = {"rays": n, "hits": hits, "any_hit": anyhit,
                          "ms": {k: round(v, 4) for k, v in med.items()},
                          "mrays_per_s": {k: round(n / (v * 1e3), 1) for k, v in med.items()},
                          "persistent_over_simple": round(med["simple"] / med["persistent"], 3),
                          "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                          "stats": st,
                          "node_records_per_ray": round(st["nodes_examined"] / n, 2),
                          "node_records_per_s_persistent": round(st["nodes_examined"] / (med["persistent"] * 1e-3), 0)}
            print(name, sname, json.dumps({k: out[sname][k] for k in ("rays", "mrays_per_s", "persistent_over_simple", "node_records_per_ray")}), flush=True)
        result["configs"][name] = {"triangles": c["n"], "camera": [c["cam"], c["quat"]], "sets": out}
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({n: {s: v["mrays_per_s"] for s, v in c["sets"].items()} for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
