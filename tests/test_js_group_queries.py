"""Every batched query of js/PathTracer.js through both of its routes: a PathTracer over a group (`devices: [0, 0]`, copy transport; the
query runs on member 0) and a plain single-context PathTracer on the same triangles give the same words in every typed array, and every
query refuses a partial record with the RangeError text it always had.  One Node child process, 256 records per query on the torus.

The three list queries also run with more matches than the first call has room for (16 entries per point or box, 4 per ray, plus 64), so
that the second call really runs: every triangle of the torus lies within rMax = 10 of every point and inside the box [-2, 2]^3.  A straight
line crosses this torus at most four times, which cannot exceed 4 * 256 + 64, so the rays of that case run along the long axis of a scene
that holds the torus twice, the second copy scaled by one half about the origin: eight crossings each."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import crossing_cases as cc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node") or "node"
JS = os.path.join(os.path.dirname(HERE), "raytracer-public_amd", "js")
N = 256

RANGE_ERRORS = {
    "traceRays": "traceRays: 8 floats per ray",
    "closestPoints": "closestPoints: 4 floats per point",
    "sweepSpheres": "sweepSpheres: 8 floats per sweep",
    "nearestK": "nearestK: 4 floats per point",
    "nearestK k = 0": "nearestK: k must be 1 .. 64",
    "nearestK k = 65": "nearestK: k must be 1 .. 64",
    "signedDistance": "signedDistance: 4 floats per point",
    "contains": "contains: 4 floats per point",
    "occlusion": "occlusion: 8 floats per surfel",
    "countHits": "countHits: 8 floats per ray",
    "radiusCount": "radiusCount: 4 floats per point",
    "boxCount": "boxCount: 8 floats per box",
    "radiusSearch": "radiusSearch: 4 floats per point",
    "boxSearch": "boxSearch: 8 floats per box",
    "listHits": "listHits: 8 floats per ray",
    "hitSurfels": "hitSurfels: 8 floats per ray and one hit per ray",
    "hitSurfels hits": "hitSurfels: 8 floats per ray and one hit per ray",
}

SCRIPT = r"""
const fs = require("fs");
const PT = require(%r);
const dir = %r;
const f32 = (name) => { const raw = fs.readFileSync(dir + name + ".f32"); return new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4); };
const tris = f32("tris"), nested = f32("nested"), rays = f32("rays"), points = f32("points"), sweeps = f32("sweeps"), boxes = f32("boxes"),
      wide = f32("wide"), along = f32("along");
const longer = (a) => { const b = new Float32Array(a.length + 1); b.set(a); return b; };
const meta = { names: {}, errors: {} };

async function run(tag, options) {
  const pt = new PT.PathTracer({ width: 64, height: 48 }, options);
  await pt.initialize();
  await pt.buildBVH(tris);
  const hits = await pt.traceRays(rays);
  const surfels = await pt.hitSurfels(rays, hits, 0.5);
  const results = {
    traceRays: hits, traceRaysAnyHit: await pt.traceRays(rays, { anyHit: true }),
    closestPoints: await pt.closestPoints(points), closestPointsSimple: await pt.closestPoints(points, { simple: true }),
    sweepSpheres: await pt.sweepSpheres(sweeps), nearestK: await pt.nearestK(points, 5, { rMax: 0.6 }),
    signedDistance: await pt.signedDistance(points, { samples: 3, seed: 2 }), contains: await pt.contains(points, { samples: 5, seed: 4 }),
    hitSurfels: { surfels: surfels }, occlusion: await pt.occlusion(surfels, { samples: 8, seed: 3 }),
    countHits: { counts: await pt.countHits(rays) }, radiusCount: { counts: await pt.radiusCount(points) }, boxCount: { counts: await pt.boxCount(boxes) },
    radiusSearch: await pt.radiusSearch(points), boxSearch: await pt.boxSearch(boxes), listHits: await pt.listHits(rays, { sort: true }),
    radiusSearchAll: await pt.radiusSearch(points, 10.0), boxSearchAll: await pt.boxSearch(wide),
  };
  const errors = {};
  const refused = async (name, call) => { try { await call(); errors[name] = ["no error", ""]; } catch (e) { errors[name] = [e.name, e.message]; } };
  await refused("traceRays", () => pt.traceRays(longer(rays)));
  await refused("closestPoints", () => pt.closestPoints(longer(points)));
  await refused("sweepSpheres", () => pt.sweepSpheres(longer(sweeps)));
  await refused("nearestK", () => pt.nearestK(longer(points), 5));
  await refused("nearestK k = 0", () => pt.nearestK(points, 0));
  await refused("nearestK k = 65", () => pt.nearestK(points, 65));
  await refused("signedDistance", () => pt.signedDistance(longer(points)));
  await refused("contains", () => pt.contains(longer(points)));
  await refused("occlusion", () => pt.occlusion(longer(surfels)));
  await refused("countHits", () => pt.countHits(longer(rays)));
  await refused("radiusCount", () => pt.radiusCount(longer(points)));
  await refused("boxCount", () => pt.boxCount(longer(boxes)));
  await refused("radiusSearch", () => pt.radiusSearch(longer(points)));
  await refused("boxSearch", () => pt.boxSearch(longer(boxes)));
  await refused("listHits", () => pt.listHits(longer(rays)));
  await refused("hitSurfels", () => pt.hitSurfels(longer(rays), hits));
  await refused("hitSurfels hits", () => pt.hitSurfels(rays, { t: hits.t.subarray(1), prim: hits.prim, u: hits.u, v: hits.v }));
  await pt.buildBVH(nested);
  results.listHitsAll = await pt.listHits(along);
  pt.destroy();
  const names = [];
  for (const [query, r] of Object.entries(results)) for (const [k, v] of Object.entries(r)) {
    const a = ArrayBuffer.isView(v) ? v : Uint32Array.of(v);                     // nearestK's k
    names.push(query + "." + k);
    fs.writeFileSync(dir + tag + "." + query + "." + k, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
  }
  meta.names[tag] = names; meta.errors[tag] = errors;
}
(async () => {
  const log = console.log; console.log = () => {};
  await run("group", { devices: [0, 0], transport: "copy" });
  await run("single", {});
  log(JSON.stringify(meta));
})().catch((e) => { console.error(e); process.exit(1); });
"""


def test_group_and_single_context_routes_give_the_same_words(tmp_path, rt):
    tris = cc.geometry(rt, "torus")
    rng = np.random.default_rng(29)
    rays = cc.ray_set(rt, tris, N, 31)
    sweeps = rays.copy(); sweeps[:, 7] = rng.uniform(0.01, 0.2, N)
    points = rt.pack_points(cc.cube_points(N, 32, 1.0), rng.uniform(0.1, 0.5, N).astype(np.float32))
    lo = cc.cube_points(N, 33, 1.0)
    boxes = rt.pack_boxes(lo, lo + rng.uniform(0.05, 0.4, (N, 3)).astype(np.float32))
    wide = rt.pack_boxes(np.full((N, 3), -2.0), np.full((N, 3), 2.0))
    along = rt.pack_rays(np.stack([np.full(N, -2.0), rng.uniform(-0.1, 0.1, N), rng.uniform(-0.03, 0.03, N)], axis=1), np.tile(np.float32([1, 0, 0]), (N, 1)))
    nested = np.concatenate([tris, np.float32(0.5) * tris])
    out = str(tmp_path) + os.sep
    for name, a in (("tris", tris), ("nested", nested), ("rays", rays), ("points", points), ("sweeps", sweeps), ("boxes", boxes), ("wide", wide), ("along", along)):
        np.ascontiguousarray(a, np.float32).tofile(out + name + ".f32")
    script = tmp_path / "queries.js"
    script.write_text(SCRIPT % (os.path.join(JS, "PathTracer.js"), out))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    meta = json.loads(r.stdout.strip().splitlines()[-1])

    def words(tag, name, dtype=np.uint32):
        return np.fromfile(out + tag + "." + name, dtype)
    names = meta["names"]["single"]
    assert meta["names"]["group"] == names and len(names) == 65, names
    for name in names:
        g, s = words("group", name, np.uint8), words("single", name, np.uint8)
        assert g.size == s.size and np.array_equal(g, s), name
    # the queries did meet the mesh, and the three large list queries did outgrow the first call's room
    for name in ("traceRays", "closestPoints", "sweepSpheres", "nearestK", "signedDistance", "radiusSearch", "boxSearch", "listHits"):
        prim = words("group", name + ".prim")
        assert prim.size >= N // 4 and (prim != cc.MISS).sum() >= N // 4, name
    assert words("group", "nearestK.k").tolist() == [5] and words("group", "nearestK.prim").size == 5 * N
    assert words("group", "contains.inside").sum() > 0 and words("group", "occlusion.unoccluded").sum() > 0 and words("group", "countHits.counts").sum() > N
    assert words("group", "radiusCount.counts").sum() > 0 and words("group", "boxCount.counts").sum() > 0
    num_tris = tris.size // 9
    for name, guess, total in (("radiusSearchAll", 16, N * num_tris), ("boxSearchAll", 16, N * num_tris), ("listHitsAll", 4, 8 * N)):
        offsets = words("group", name + ".offsets", np.float64)
        assert offsets.size == N + 1 and offsets[N] == total and offsets[N] > guess * N + 64, (name, offsets[N])
        assert words("group", name + ".prim").size == total
    for tag in ("group", "single"):
        assert meta["errors"][tag] == {name: ["RangeError", text] for name, text in RANGE_ERRORS.items()}, tag
