"""The Node route of the hit lists: PathTracer.listHits and hitsAlong give the Python results bit for bit on tetra and torus, and
`main.js --thickness` writes a frame whose non-black pixels are t[1] - t[0] of the host twin's sorted lists of the camera rays."""
import json
import os
import subprocess

import numpy as np
import pytest

import crossing_cases as cc
import hitlist_cases as hc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = "/usr/bin/node" if os.path.exists("/usr/bin/node") else "node"
JS = os.path.join(os.path.dirname(HERE), "raytracer-public_amd", "js")
SCENE_SEED = 20260109
W, H = 64, 48


def test_node_list_hits_hits_along_and_thickness(tmp_path, rt, gpu_ctx):
    names = ["tetra", "torus"]
    for name in names:
        tris = cc.geometry(rt, name)
        tris.tofile(str(tmp_path / (name + "_tris.f32")))
        cc.ray_set(rt, tris, 2048, 11).tofile(str(tmp_path / (name + "_rays.f32")))
    script = tmp_path / "hl.js"
    script.write_text("""
const fs = require("fs");
const PT = require(%r);
const dir = %r;
const f32 = (p) => { const raw = fs.readFileSync(p); return new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4); };
const save = (name, o) => { for (const [k, v] of Object.entries(o)) fs.writeFileSync(dir + name + "_" + k, Buffer.from(v.buffer, v.byteOffset, v.byteLength)); };
(async () => {
  const pt = new PT.PathTracer({ width: %d, height: %d });
  await pt.initialize();
  for (const name of %s) {
    await pt.buildBVH(f32(dir + name + "_tris.f32"));
    const rays = f32(dir + name + "_rays.f32");
    const s = await pt.listHits(rays, { sort: true });
    const visit = await pt.listHits(rays, { simple: true });
    const brute = await pt.listHits(rays, { bruteForce: true });
    const one = await pt.hitsAlong(rays[0], rays[1], rays[2], rays[4], rays[5], rays[6]);
    save(name, { offsets: s.offsets, t: s.t, prim: s.prim, u: s.u, v: s.v, visit_offsets: visit.offsets, visit_t: visit.t, visit_prim: visit.prim,
                 brute_offsets: brute.offsets, brute_prim: brute.prim, one_t: one.t, one_prim: one.prim, one_count: Uint32Array.of(one.count) });
  }
  // the camera rays of the driver's default camera over its stand-in scene, and the thickness frame of the same
  await pt.buildBVH(PT.native().proceduralScene(0, 20000, %d));
  pt.setCameraPosition(0, 0, 2.5); pt.setCameraQuaternion(0, 0, 0, 1);
  const ubo = pt._ubo(), cam = new Float32Array(%d * %d * 8);
  for (let y = 0; y < %d; y++) for (let x = 0; x < %d; x++) cam.set(PT.native().cameraRay(ubo, x, y), (y * %d + x) * 8);
  save("cam", { rays: cam, thickness: await pt.thickness() });
  pt.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
""" % (os.path.join(JS, "PathTracer.js"), str(tmp_path) + os.sep, W, H, json.dumps(names), SCENE_SEED, W, H, H, W, W))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr

    def out(name, k, dt=np.uint32):
        return np.fromfile(str(tmp_path / (name + "_" + k)), dt)
    for name in names:
        tris = cc.geometry(rt, name)
        rays = cc.ray_set(rt, tris, 2048, 11)
        gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
        want = gpu_ctx.list_hits(rays, sort=True)
        assert int(want[0][-1]) > len(rays) // 2
        got = (out(name, "offsets", np.float64).astype(np.uint64), out(name, "t", np.float32), out(name, "prim"), out(name, "u", np.float32), out(name, "v", np.float32))
        hc.assert_same_lists(got, want)
        hc.assert_same_lists(got, rt.list_hits_bvh4(tris, gpu_ctx.read_bvh4(), rays, sort=True))
        visit = gpu_ctx.list_hits(rays)
        assert np.array_equal(out(name, "visit_offsets", np.float64).astype(np.uint64), visit[0]) and np.array_equal(out(name, "visit_prim"), visit[2])
        assert np.array_equal(hc.bits(out(name, "visit_t", np.float32)), hc.bits(visit[1]))
        brute = gpu_ctx.list_hits(rays, brute_force=True)
        assert np.array_equal(out(name, "brute_offsets", np.float64).astype(np.uint64), brute[0]) and np.array_equal(out(name, "brute_prim"), brute[2])
        a, b = int(want[0][0]), int(want[0][1])
        assert out(name, "one_count")[0] == b - a and np.array_equal(out(name, "one_prim"), want[2][a:b])
        assert np.array_equal(hc.bits(out(name, "one_t", np.float32)), hc.bits(want[1][a:b]))

    # the driver: --thickness over the stand-in scene, the frame's floats against the twin on the same camera rays
    frame = tmp_path / "thick.f32"
    r = subprocess.run([NODE, os.path.join(JS, "main.js"), "--tris", "20000", "--mode", "1", "--frames", "1", "--width", str(W), "--height", str(H),
                        "--dump", str(tmp_path / "d" / "BVH2.bin"), "--thickness", "--radiance", str(frame)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    line = next(json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and "thickness" in l)
    big = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000, SCENE_SEED)
    gpu_ctx.set_triangles(big); gpu_ctx.build_bvh()
    cam = out("cam", "rays", np.float32).reshape(-1, 8)
    twin = rt.list_hits_bvh4(big, gpu_ctx.read_bvh4(), cam, sort=True)
    off = twin[0].astype(np.int64)
    two = np.diff(off) >= 2
    want = np.zeros(W * H, np.float32)
    want[two] = twin[1][off[:-1][two] + 1] - twin[1][off[:-1][two]]
    img = np.fromfile(str(frame), np.float32).reshape(-1, 4)
    assert 0 < two.sum() < W * H and line["pixelsWithTwoHits"] == int((want > 0).sum())
    for c in range(3):
        assert np.array_equal(hc.bits(img[:, c]), hc.bits(want))          # t[1] - t[0] where there are two hits, black elsewhere
    assert np.all(img[:, 3] == 1)
    assert np.array_equal(hc.bits(out("cam", "thickness", np.float32)), hc.bits(want))
