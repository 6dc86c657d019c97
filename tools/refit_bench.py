#!/usr/bin/env python3
"""Refit in place against rebuilding (pt_update_triangles) on one GPU, in one process, alternating.

Scenes C2 (dragon-class, 871,414 triangles) and C4 (sponza-class interior, 262,144), build levels 0 and 2, the drivers' `--animate`
displacement (tools/README.md) at amplitudes 0.02 and 0.1.  Per case, the median of --reps (5) timings, host wall clock around the call
plus a synchronise, in ms:

    update_device_ms     update_triangles from a device tensor (copy, triangle records, refit; no upload)
    update_host_ms       update_triangles from a host array (with the 36 B / triangle upload)
    build_ms             build_bvh(level) alone, the new triangles already uploaded
    set_and_build_ms     set_triangles + build_bvh(level): the whole path without this feature
    prepare_ms           the first update after a build (it also derives the parent links), once per case

and ms/frame of the next batched 1920x1080 / 4 spp / 8-bounce launch on the refitted tree and on the rebuilt tree, with bvh_cost of
both and of the tree as built.  The gates of the feature are evaluated per case: update_device_ms < build_ms at level 0, and
update_device_ms < build_ms / 2 at level 2.

    python tools/refit_bench.py [--reps 5] [--out profiles/refit_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch      # before the package: both must drive the GPU through one copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
import importlib  # noqa: E402

W, H, SPP, BOUNCES, SEED, SCENE_SEED = 1920, 1080, 4, 8, 1, 20260109
LEVELS = (0, 2)
AMPS = (0.02, 0.1)
CONFIGS = {
    "C2": dict(kind=0, n=871414, cam=(0, 0, 2.5), quat=(0, 0, 0, 1), frames=32),
    "C4": dict(kind=1, n=262144, cam=(0.55, -0.05, 0.05), quat=(0.0, 0.6630, 0.0, 0.7486), frames=8),
}
f32 = np.float32


def wave(tris, amp, frame):
    """main.js --animate AMP at `frame` (tools/README.md), every step rounded to f32"""
    v = np.array(tris, f32).reshape(-1, 3)
    u = ((f32(2) * v[:, 0]).astype(f32) + f32(0.25)).astype(f32) + f32(f32(0.125) * f32(frame))
    d = ((u - np.floor(u)).astype(f32) - f32(0.5)).astype(f32)
    v[:, 1] = (v[:, 1] + (f32(amp) * ((f32(4) * np.abs(d)).astype(f32) - f32(1)).astype(f32)).astype(f32)).astype(f32)
    return v.reshape(-1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rt = importlib.import_module("raytracer-public_amd")
    frame = [1000]

    def timed(ctx, fn):
        ctx.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def launch(ctx, c):
        p = ctx.make_params(W, H, c["cam"], c["quat"], mode=rt.PT_MODE_PATH, spp=SPP, max_bounces=BOUNCES, seed=SEED)
        ctx.set_batch(c["frames"])
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(c["frames"]):
            p.frame = frame[0]; frame[0] += 1
            ctx.render(p)
        ctx.synchronize()
        ctx.set_batch(1)
        return (time.perf_counter() - t0) * 1e3 / c["frames"]

    med = lambda v: round(statistics.median(v), 4)
    result = {"resolution": [W, H], "spp": SPP, "max_bounces": BOUNCES, "reps": args.reps, "cases": []}
    for name, c in CONFIGS.items():
        base = rt.procedural_scene(c["kind"], c["n"], SCENE_SEED)
        base_t = torch.from_numpy(base).cuda()
        for lvl in LEVELS:
            refit, rebuilt = rt.Context(0), rt.Context(0)
            refit.set_triangles(base); refit.build_bvh(lvl)
            rebuilt.set_triangles(base); rebuilt.build_bvh(lvl)
            built_cost = refit.bvh_cost()
            refit.build_bvh(lvl)                               # a fresh tree: the first update after it derives the parent links, timed as prepare_ms
            prepare_ms = timed(refit, lambda: refit.update_triangles(base_t))
            launch(refit, c); launch(rebuilt, c)               # warm-up
            for amp in AMPS:
                moved = wave(base, amp, 1)
                moved_t = torch.from_numpy(moved).cuda()
                t = {k: [] for k in ("update_device_ms", "update_host_ms", "build_ms", "set_and_build_ms", "refit_ms_per_frame", "rebuilt_ms_per_frame")}
                for rep in range(args.reps + 1):               # the first round warms up
                    row = {}
                    refit.update_triangles(base_t)
                    row["update_device_ms"] = timed(refit, lambda: refit.update_triangles(moved_t))
                    refit.update_triangles(base_t)
                    row["update_host_ms"] = timed(refit, lambda: refit.update_triangles(moved))
                    rebuilt.set_triangles(moved)
                    row["build_ms"] = timed(rebuilt, lambda: rebuilt.build_bvh(lvl))
                    row["set_and_build_ms"] = timed(rebuilt, lambda: (rebuilt.set_triangles(moved), rebuilt.build_bvh(lvl)))
                    row["refit_ms_per_frame"] = launch(refit, c)
                    row["rebuilt_ms_per_frame"] = launch(rebuilt, c)
                    if rep:
                        for k, v in row.items():
                            t[k].append(v)
                case = {"config": name, "triangles": c["n"], "level": lvl, "amp": amp, "num_nodes4": refit.scene_info()["numNodes4"],
                        "prepare_ms": round(prepare_ms, 4), "bvh_cost_at_build": built_cost, "bvh_cost_refit": refit.bvh_cost(), "bvh_cost_rebuilt": rebuilt.bvh_cost()}
                case.update({k: med(v) for k, v in t.items()})
                case["min_max"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
                case["frame_time_refit_over_rebuilt"] = round(case["refit_ms_per_frame"] / case["rebuilt_ms_per_frame"], 4)
                bound = case["build_ms"] if lvl == 0 else case["build_ms"] / 2
                case["gate"] = "update_device_ms < build_ms" + ("" if lvl == 0 else " / 2")
                case["gate_met"] = bool(case["update_device_ms"] < bound)
                result["cases"].append(case)
                print(json.dumps(case), flush=True)
            refit.close(); rebuilt.close()
    result["gates_met"] = all(c["gate_met"] for c in result["cases"])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({"gates_met": result["gates_met"]}))


if __name__ == "__main__":
    main()
