#!/usr/bin/env python3
"""Throughput of the k-nearest queries (include/mi355pt.h pt_nearest_k): the persistent kernel (the capacity tiers
4, 16 and 64 of nearest_k_kernel<KCAP>) against the simple one-point-per-thread kernel, and k = 1 against pt_closest_points on the same
points, in one process, kernels alternating, on C2 (dragon-class, 871,414 triangles) and C4 (sponza-class interior, 262,144 triangles),
each at build level 0 and 2.

Point sets: the three of tools/pointquery_bench.py (surface, box, far), the first 262,144 points of each, in device memory (torch
tensors, zero-copy), r_max = +inf, so every row is full.
Per set, k in (1, 4, 16, 64) and kernel: the median over --reps launches (after one warm-up) of the launch time by events on the
context's stream, in Mpoints/s and Mrecords/s (n * k records are written); persistent_over_simple = ms(simple) / ms(persistent).  For
k = 1 also closest_points on the same points and nearest_over_closest = ms(nearest_k, k = 1) / ms(closest_points): what the list in LDS and
the smaller grid cost where they buy nothing.  Per set and k: node records and triangles per point, stack_drops and max_stack from one
PT_NEAREST_STATS pass.  There is no gate: the query has no predecessor.

    python tools/knn_bench.py [--reps 5] [--out profiles/knn_ab.json]      (--out defaults to that file)
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

N_POINTS = 262144
KS = (1, 4, 16, 64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_ab.json"))
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("raytracer-public_amd")
    stream = torch.cuda.current_stream()
    result = {"tool": "tools/knn_bench.py", "reps": args.reps, "device": torch.cuda.get_device_name(0), "points": N_POINTS,
              "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "configs": {}}
    for name, c in pq.CONFIGS.items():
        tris = rt.procedural_scene(c["kind"], c["n"], pq.SCENE_SEED)
        sets = {k: torch.from_numpy(rt.pack_points(p[:N_POINTS])).cuda() for k, p in pq.point_sets(tris, np.random.default_rng(pq.RNG_SEED)).items()}
        for accel in pq.ACCELS:
            ctx = rt.Context(0)
            ctx.set_triangles(tris); ctx.build_bvh(accel)
            ctx.set_stream(stream.cuda_stream)               # launches straight on torch's stream: the events time the kernels alone
            out = {}
            for sname, pts in sets.items():
                n = pts.shape[0]
                for k in KS:
                    ms = {"persistent": [], "simple": []}
                    if k == 1:
                        ms["closest_points"] = []
                    for rep in range(args.reps + 1):
                        for kernel in ("persistent", "simple"):
                            t, res = pq.timed(torch, stream, lambda: ctx.nearest_k(pts, k, simple=kernel == "simple"))
                            if rep:
                                ms[kernel].append(t)
                            got = torch.stack([x.contiguous().view(torch.int32) for x in res])
                            if kernel == "persistent":
                                ref = got
                            else:
                                assert torch.equal(ref, got), "the kernels disagree"
                            del got
                        if k == 1:
                            t, res = pq.timed(torch, stream, lambda: ctx.closest_points(pts))
                            if rep:
                                ms["closest_points"].append(t)
                            assert torch.equal(ref[:, :, 0], torch.stack([x.view(torch.int32) for x in res])), "k = 1 and closest_points disagree"
                    del ref
                    ctx.nearest_k(pts, k, stats=True)
                    st = ctx.stats()
                    med = {w: statistics.median(x) for w, x in ms.items()}
                    key = "%s_k%d" % (sname, k)
                    out[key] = {"points": n, "k": k, "ms": {w: round(x, 4) for w, x in med.items()},
                                "mpoints_per_s": {w: round(n / (x * 1e3), 1) for w, x in med.items()},
                                "mrecords_per_s": {w: round(n * k / (med[w] * 1e3), 1) for w in ("persistent", "simple")},
                                "persistent_over_simple": round(med["simple"] / med["persistent"], 3),
                                "ms_all": {w: [round(x, 4) for x in v] for w, v in ms.items()},
                                "stats": st,
                                "node_records_per_point": round(st["nodes_examined"] / n, 2),
                                "triangles_per_point": round(st["tris_tested"] / n, 2)}
                    if k == 1:
                        out[key]["nearest_over_closest"] = round(med["persistent"] / med["closest_points"], 3)
                    print(name, "accel", accel, key, json.dumps({w: out[key][w] for w in ("mpoints_per_s", "persistent_over_simple", "node_records_per_point", "triangles_per_point")}),
                          "drops", st["stack_drops"], "max_stack", st["max_stack"], flush=True)
            result["configs"]["%s_accel%d" % (name, accel)] = {"triangles": c["n"], "accel": accel, "sets": out}
            ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({n: {s: v["mpoints_per_s"]["persistent"] for s, v in c["sets"].items()} for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
