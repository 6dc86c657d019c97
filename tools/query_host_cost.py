"""Host cost of the batched queries' front end: microseconds per call of trace_rays_device, closest_points_device, radius_search_device and
list_hits_device with n = 64 on a 20-triangle scene, where the launch is nothing and the host side of the call is everything.  No host wait
between calls; the median over QH_REPS repetitions of QH_CALLS calls each.  Then the numpy host route of the same four (trace_rays,
closest_points, radius_search and list_hits with a capacity) over the same records: the Python binding's packing, staging and unpacking,
each call with its one host wait by design.  Prints one JSON line.  PB_BASE=1: the library of an earlier
commit (tools/ab/README), for an A/B within one session -- numbers of different sessions do not compare."""
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if os.environ.get("PB_BASE"):
    sys.path.insert(0, os.path.join(ROOT, "tools", "ab")); rt = importlib.import_module("raytracer_base")
else:
    rt = importlib.import_module("raytracer-public_amd")
CALLS, REPS, N = int(os.environ.get("QH_CALLS", 3000)), int(os.environ.get("QH_REPS", 7)), 64

hip = C.CDLL("libamdhip64.so")


def device(nbytes, host=None):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
    if host is not None:
        assert hip.hipMemcpy(p, C.c_void_p(host.ctypes.data), C.c_size_t(host.nbytes), C.c_int(1)) == 0
    return p.value


# ten unit quads stacked along z; rays down -z through all of them, points beside them
z = np.linspace(-2.0, 2.0, 10, dtype=np.float32)
quad = lambda zz: [[-.5, -.5, zz, .5, -.5, zz, .5, .5, zz], [-.5, -.5, zz, .5, .5, zz, -.5, .5, zz]]
tris = np.float32([t for zz in z for t in quad(zz)]).reshape(-1)
rng = np.random.default_rng(1)
xy = rng.uniform(-0.4, 0.4, (N, 2)).astype(np.float32)
org = np.concatenate([xy, np.full((N, 1), 3.0, np.float32)], 1)
host_rays, host_points = rt.pack_rays(org, np.tile(np.float32([0, 0, -1]), (N, 1))), rt.pack_points(org, 10.0)
rays, points = device(N * 32, host_rays), device(N * 16, host_points)
out, offsets, entries = device(N * 16), device((N + 1) * 8), device(2048 * 16)      # at most 20 entries per list

ctx = rt.Context(0); ctx.set_triangles(tris); ctx.build_bvh()
queries = {
    "trace_rays_device": lambda: ctx.trace_rays_device(rays, N, out),
    "closest_points_device": lambda: ctx.closest_points_device(points, N, out),
    "radius_search_device": lambda: ctx.radius_search_device(points, N, offsets, entries, 2048),
    "list_hits_device": lambda: ctx.list_hits_device(rays, N, offsets, entries, 2048),
    "trace_rays_host": lambda: ctx.trace_rays(host_rays),
    "closest_points_host": lambda: ctx.closest_points(host_points),
    "radius_search_host": lambda: ctx.radius_search(host_points, capacity=2048),
    "list_hits_host": lambda: ctx.list_hits(host_rays, capacity=2048),
}
result = {"build": "base" if os.environ.get("PB_BASE") else "tree", "n": N, "calls": CALLS, "reps": REPS}
for name, call in queries.items():
    for _ in range(200):
        call()
    ctx.synchronize()
    us = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        us.append((time.perf_counter() - t0) / CALLS * 1e6)
        ctx.synchronize()
    result[name] = round(statistics.median(us), 3)
ctx.close()
print(json.dumps(result))
