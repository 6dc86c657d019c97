"""PathTracer.sweepSpheres and sweep (raytracer-public_amd/js/PathTracer.js over the N-API addon) give the Python host route's bits on the
tetrahedron and on the torus."""
import os
import subprocess

import numpy as np
import pytest

import crossing_cases as cc
import sweep_cases as sc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = "/usr/bin/node" if os.path.exists("/usr/bin/node") else "node"
JS = os.path.join(os.path.dirname(HERE), "raytracer-public_amd", "js")


@pytest.mark.parametrize("name", ["tetra", "torus"])
def test_node_sweeps(tmp_path, rt, gpu_ctx, name):
    tris = cc.geometry(rt, name)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    sweeps = sc.sweep_set(rt, tris, 2048, 17)
    sweeps[:, 3] = np.inf                                                 # sweep() takes no tMax
    sweeps.tofile(str(tmp_path / "sweeps.f32"))
    np.ascontiguousarray(tris, np.float32).tofile(str(tmp_path / "tris.f32"))
    script = tmp_path / "sweep.js"
    script.write_text("""
const fs = require("fs");
const PT = require(%r);
const f32 = (p) => { const raw = fs.readFileSync(p); return new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4); };
(async () => {
  const pt = new PT.PathTracer({ width: 64, height: 48 });
  await pt.initialize();
  await pt.buildBVH(f32(%r));
  const sw = f32(%r);
  const s = await pt.sweepSpheres(sw);
  const simple = await pt.sweepSpheres(sw, { simple: true });
  const brute = await pt.sweepSpheres(sw, { bruteForce: true });
  const k = 8 * 1500;
  const one = await pt.sweep(sw[k], sw[k + 1], sw[k + 2], sw[k + 4], sw[k + 5], sw[k + 6], sw[k + 7]);
  const out = { t: s.t, prim: s.prim, u: s.u, v: s.v, simple_t: simple.t, simple_prim: simple.prim, brute_t: brute.t, brute_u: brute.u,
                one_t: Float32Array.of(one.t, one.u, one.v), one_prim: Uint32Array.of(one.prim, one.hit ? 1 : 0) };
  for (const [k, v] of Object.entries(out)) fs.writeFileSync(%r + k, Buffer.from(v.buffer, v.byteOffset, v.byteLength));
  pt.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
""" % (os.path.join(JS, "PathTracer.js"), str(tmp_path / "tris.f32"), str(tmp_path / "sweeps.f32"), str(tmp_path / "out_")))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr

    def out(k, dt=np.uint32):
        return np.fromfile(str(tmp_path / ("out_" + k)), dt)
    want = gpu_ctx.sweep_spheres(sweeps)
    assert (want[1] != sc.MISS).sum() > 1024
    for k, col in enumerate(("t", "prim", "u", "v")):
        assert np.array_equal(out(col), sc.bits(want[k])), col
    assert np.array_equal(out("simple_t"), sc.bits(want[0])) and np.array_equal(out("simple_prim"), want[1])
    brute = gpu_ctx.sweep_spheres(sweeps, brute_force=True)
    assert np.array_equal(out("brute_t"), sc.bits(brute[0])) and np.array_equal(out("brute_u"), sc.bits(brute[2]))
    one = gpu_ctx.sweep_spheres(sweeps[1500:1501])
    assert np.array_equal(out("one_t"), np.concatenate([sc.bits(one[0]), sc.bits(one[2]), sc.bits(one[3])]))
    assert out("one_prim")[0] == one[1][0] and out("one_prim")[1] == int(one[1][0] != sc.MISS)
