"""Batched ray queries (pt_trace_rays / pt_trace_rays_host / pt_camera_rays) against the CPU oracle's
single-ray traversal (oracle/pt_oracle.cpp::orc_trace_ray): t bits, prim and the hit flag, closest and any hit, both kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orc as orc_mod
from routecheck import run_case
from scenes import TETRA, comb_bvh4, random_soup, spoil_bvh4

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE_SEED = 20260109
MISS = 0xFFFFFFFF
KERNELS = [False, True]       # simple=False: the persistent kernel; True: the one-ray-per-thread kernel


def oracle_batch(orc, tris, bvh4, O, D, anyhit=False):
    hit = np.zeros(len(O), bool); t = np.full(len(O), np.inf, np.float32); prim = np.full(len(O), MISS, np.uint32)
    for i in range(len(O)):
        h, tt, _, tri = orc.trace_ray(tris, bvh4, O[i], D[i], anyhit=anyhit)
        if h:
            hit[i], t[i], prim[i] = True, tt, tri
    return hit, t, prim


def random_rays(tris, n, seed):
    """Origins inside and outside the scene and on its surface; unnormalised directions, every 8th axis-parallel."""
    rng = np.random.default_rng(seed)
    T = tris.reshape(-1, 3, 3)
    lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
    k = n // 4
    inside = lo + rng.random((k, 3), dtype=np.float32) * (hi - lo)
    outside = rng.normal(size=(k, 3)).astype(np.float32)
    outside = outside / np.linalg.norm(outside, axis=1, keepdims=True) * np.float32(3.0)
    pick = rng.integers(0, len(T), k)
    b = rng.random((k, 2), dtype=np.float32); b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    surface = T[pick, 0] + b[:, :1] * (T[pick, 1] - T[pick, 0]) + b[:, 1:] * (T[pick, 2] - T[pick, 0])
    far = rng.uniform(-4, 4, (n - 3 * k, 3)).astype(np.float32)
    O = np.concatenate([inside, outside, surface, far]).astype(np.float32)
    target = lo + rng.random((n, 3), dtype=np.float32) * (hi - lo)
    D = rng.normal(size=(n, 3)).astype(np.float32)
    D[k:2 * k] = target[k:2 * k] - O[k:2 * k]                 # from outside towards the scene
    D *= rng.uniform(0.1, 10.0, (n, 1)).astype(np.float32)
    ax = np.arange(0, n, 8)
    D[ax] = 0.0
    D[ax, rng.integers(0, 3, len(ax))] = (rng.choice([-1.0, 1.0], len(ax)) * rng.uniform(0.5, 2, len(ax))).astype(np.float32)
    return O, D.astype(np.float32)


def check_against_oracle(orc, ctx, tris, bvh4, O, D, anyhit, simple, sub=None):
    t, prim, u, v = ctx.trace_rays(O, D, any_hit=anyhit, simple=simple)
    idx = np.arange(len(O)) if sub is None else sub
    hit, ot, oprim = oracle_batch(orc, tris, bvh4, O[idx], D[idx], anyhit)
    got_hit = prim[idx] != MISS
    assert np.array_equal(got_hit, hit), np.flatnonzero(got_hit != hit)[:10]
    assert np.array_equal(prim[idx][hit], oprim[hit])
    assert np.array_equal(t[idx][hit].view(np.uint32), ot[hit].view(np.uint32))
    assert np.all(np.isposinf(t[idx][~hit])) and np.all(u[idx][~hit] == 0) and np.all(v[idx][~hit] == 0)
    return t, prim, u, v


def scene(rt, ctx, name, accel=0):
    if name == "tetra":
        tris = TETRA
    elif name == "soup1k":
        tris = random_soup(1000, 3)
    elif name == "soup120k":
        tris = random_soup(120000, 5, size=0.02)
    else:
        tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 871414, SCENE_SEED)
    ctx.set_triangles(tris)
    ctx.build_bvh(accel)
    return tris, ctx.read_bvh4()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("anyhit", [False, True])
@pytest.mark.parametrize("simple", KERNELS)
@pytest.mark.parametrize("name", ["tetra", "soup1k", "soup120k"])
def test_queries_equal_the_oracle(rt, orc, gpu_ctx, name, simple, anyhit):
    tris, bvh4 = scene(rt, gpu_ctx, name)
    O, D = random_rays(tris, 20000, 7)
    check_against_oracle(orc, gpu_ctx, tris, bvh4, O, D, anyhit, simple)


@pytest.mark.parametrize("accel", [0, 1, 2])
def test_queries_on_every_accel_level(rt, orc, gpu_ctx, accel):
    tris, bvh4 = scene(rt, gpu_ctx, "soup120k", accel)
    O, D = random_rays(tris, 20000, 11)
    for simple in KERNELS:
        for anyhit in (False, True):
            check_against_oracle(orc, gpu_ctx, tris, bvh4, O, D, anyhit, simple)


def test_full_size_dragon(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "dragon")
    O, D = random_rays(tris, 200000, 13)
    sub = np.sort(np.random.default_rng(1).choice(len(O), 2000, replace=False))
    res = [check_against_oracle(orc, gpu_ctx, tris, bvh4, O, D, False, simple, sub=sub) for simple in KERNELS]
    for a, b in zip(res[0], res[1]):              # persistent == simple on every ray, not only the oracle's subset
        assert same_bits(a, b)
    check_against_oracle(orc, gpu_ctx, tris, bvh4, O, D, True, False, sub=sub)


def test_barycentrics_restate_moller_trumbore(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "soup1k")
    O, D = random_rays(tris, 20000, 17)

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    for simple in KERNELS:
        t, prim, u, v = gpu_ctx.trace_rays(O, D, simple=simple)
        h = np.flatnonzero(prim != MISS)
        assert len(h) > 1000
        T = tris.reshape(-1, 3, 3)[prim[h]]
        v0 = T[:, 0]; e1 = T[:, 1] - T[:, 0]; e2 = T[:, 2] - T[:, 0]      # the triangle record's edges (pt_host.h::TriRecord), f32
        d, o = D[h], O[h]
        p = cross(d, e2); det = dot(e1, p); inv = np.float32(1.0) / det
        s = o - v0; uu = inv * dot(s, p); q = cross(s, e1); vv = inv * dot(d, q); tt = inv * dot(e2, q)
        assert uu.dtype == np.float32
        assert same_bits(u[h], uu) and same_bits(v[h], vv) and same_bits(t[h], tt)


def test_t_max_and_rays_without_traversal(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "soup1k")
    O, D = random_rays(tris, 8000, 19)
    hit, ot, oprim = oracle_batch(orc, tris, bvh4, O, D)
    rng = np.random.default_rng(3)
    tmax = np.where(hit, ot * rng.choice(np.float32([0.5, 1.5]), len(O)), rng.uniform(0.1, 10, len(O))).astype(np.float32)
    i0 = int(np.flatnonzero(hit)[0])                 # a ray that hits; five spoilt copies of it, then itself
    bad = np.tile(np.concatenate([O[i0], [np.inf], D[i0], [0]]).astype(np.float32), (6, 1))
    bad[0, 1] = np.nan; bad[1, 6] = np.nan; bad[2, 3] = np.nan; bad[3, 3] = 0.0; bad[4, 3] = -1.0
    for simple in KERNELS:
        t, prim, _, _ = gpu_ctx.trace_rays(O, D, t_max=tmax, simple=simple)
        want = hit & (ot < tmax)
        assert 0 < want.sum() < hit.sum()
        assert np.array_equal(prim != MISS, want)
        assert np.array_equal(prim[want], oprim[want]) and same_bits(t[want], ot[want])
        t, prim, u, v = gpu_ctx.trace_rays(bad, simple=simple)
        assert list(prim[:5]) == [MISS] * 5 and np.all(np.isposinf(t[:5])) and np.all(u[:5] == 0) and np.all(v[:5] == 0)
        assert prim[5] == oprim[i0] and same_bits(t[5:], ot[i0:i0 + 1])


@pytest.mark.parametrize("levels", [12, 30])
def test_stack_cap_scenes(rt, orc, gpu_ctx, levels):
    tris, bvh4 = comb_bvh4(levels, 5)
    gpu_ctx.set_triangles(tris); gpu_ctx.set_bvh4(bvh4)
    rng = np.random.default_rng(levels)
    n = 4000
    O = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), np.full((n, 1), 2.0)], 1).astype(np.float32)
    D = np.concatenate([rng.normal(0, 0.05, (n, 2)), -np.ones((n, 1))], 1).astype(np.float32)
    for simple in KERNELS:
        for anyhit in (False, True):
            check_against_oracle(orc, gpu_ctx, tris, bvh4, O, D, anyhit, simple)
    gpu_ctx.trace_rays(O, D, stats=True)
    drops = gpu_ctx.stats()["stack_drops"]
    assert (drops > 0) == (levels == 30), drops          # the 64-entry cap is reached on the deep comb only


def test_damaged_tree(rt, orc, gpu_ctx):
    tris = random_soup(3000, 23)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    bvh4, n_oob, n_deg = spoil_bvh4(gpu_ctx.read_bvh4(), 9)
    assert n_oob > 0 and n_deg > 0
    gpu_ctx.set_bvh4(bvh4)
    O, D = random_rays(tris, 20000, 29)
    for simple in KERNELS:
        for anyhit in (False, True):
            check_against_oracle(orc, gpu_ctx, tris, bvh4, O, D, anyhit, simple)


def test_bvh2_scene(rt, orc, gpu_ctx):
    tris = random_soup(2000, 31)
    bvh2, _ = orc.build_bvh4(tris)
    gpu_ctx.set_triangles(tris); gpu_ctx.set_bvh2(bvh2)
    O, D = random_rays(tris, 8000, 37)
    check_against_oracle(orc, gpu_ctx, tris, gpu_ctx.read_bvh4(), O, D, False, False)


@pytest.mark.parametrize("n", [0, 1, 63, 65, (1 << 20) + 3])
def test_batch_shapes(rt, orc, gpu_ctx, n):
    tris, bvh4 = scene(rt, gpu_ctx, "soup1k")
    O, D = random_rays(tris, max(n, 8), 41)
    O, D = O[:n], D[:n]
    a = gpu_ctx.trace_rays(O, D)
    b = gpu_ctx.trace_rays(O, D, simple=True)
    for x, y in zip(a, b):
        assert len(x) == n and same_bits(x, y)
    if n:
        sub = np.unique(np.linspace(0, n - 1, min(n, 300)).astype(np.int64))
        check_against_oracle(orc, gpu_ctx, tris, bvh4, O, D, False, False, sub=sub)


@pytest.mark.parametrize("case", ["camera_rays_equal_a_mode_1_render_on_c2", "ordering_with_batched_frames_and_scene_changes",
                                  "torch_route_equals_the_host_route", "errors"])
def test_torch_route(case):
    """Camera rays vs a mode-1 render of C2 (prim on every pixel, the oracle's counters), ordering behind pt_set_batch frames and before
    scene changes, the zero-copy torch route vs the host route, every error code: tests/rayquery_torch_cases.py in a child process."""
    run_case("rayquery_torch_cases", case)


def test_torch_route_needs_torch_first():
    """With the package imported before torch, the torch route says what to do instead of failing inside torch (child process)."""
    prog = ("import importlib, sys; sys.path[:0] = [%r, %r]; rt = importlib.import_module('raytracer-public_amd'); import torch\n"
            "from scenes import TETRA\n"
            "ctx = rt.Context(0); ctx.set_triangles(TETRA); ctx.build_bvh()\n"
            "try:\n    ctx.trace_rays(torch.zeros((4, 8)))\nexcept RuntimeError as e:\n    assert 'import torch' in str(e), e; print('refused')\n"
            "ctx.close()\n") % (os.path.dirname(HERE), HERE)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, cwd=HERE)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "refused" in r.stdout


NODE = "/usr/bin/node" if os.path.exists("/usr/bin/node") else "node"
JS = os.path.join(os.path.dirname(HERE), "raytracer-public_amd", "js")


def test_node_pick_and_trace_rays(tmp_path, rt, orc, gpu_ctx):
    """PathTracer.pick(x, y) at 64 pixels is the oracle's mode-1 tri_ids there; PathTracer.traceRays gives the Python results bit for bit;
    `main.js --pick X,Y` prints one JSON line."""
    w, h = 64, 48
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000, 7)
    O, D = random_rays(tris, 3000, 59)
    rays = rt.pack_rays(O, D)
    rays.tofile(str(tmp_path / "rays.f32"))
    script = tmp_path / "rq.js"
    script.write_text("""
const fs = require("fs");
const PT = require(%r);
(async () => {
  const tris = PT.native().proceduralScene(0, 20000, 7);
  const pt = new PT.PathTracer({ width: %d, height: %d });
  await pt.initialize();
  await pt.buildBVH(tris);
  pt.setCameraPosition(0, 0, 2.5);
  const picks = [];
  for (let y = 1; y < %d; y += 6) for (let x = 3; x < %d; x += 8) { const p = await pt.pick(x, y); picks.push([x, y, p.hit, p.prim, p.t, p.point]); }
  const raw = fs.readFileSync(%r);
  const r = await pt.traceRays(new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4));
  const a = await pt.traceRays(new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4), { anyHit: true });
  for (const [k, v] of Object.entries({ t: r.t, prim: r.prim, u: r.u, v: r.v, at: a.t, aprim: a.prim })) fs.writeFileSync(%r + k, Buffer.from(v.buffer));
  console.log(JSON.stringify(picks));
  pt.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
""" % (os.path.join(JS, "PathTracer.js"), w, h, h, w, str(tmp_path / "rays.f32"), str(tmp_path / "out_")))
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    picks = __import__("json").loads(r.stdout.strip().splitlines()[-1])
    assert len(picks) == 64
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    bvh4 = gpu_ctx.read_bvh4()
    _, ids, _ = orc.render(orc.make_params(w, h, 20000, cam_pos=(0, 0, 2.5), mode=orc_mod.MODE_SINGLE), tris, bvh4, want_tri_ids=True)
    assert [p[3] for p in picks] == [int(ids[y, x]) for x, y, *_ in picks]
    assert any(p[2] for p in picks) and not all(p[2] for p in picks)
    assert all((p[5] is not None) == p[2] for p in picks)
    for anyhit, keys in ((False, ("t", "prim", "u", "v")), (True, ("at", "aprim"))):
        want = gpu_ctx.trace_rays(O, D, any_hit=anyhit)
        for k, x in zip(keys, want):
            assert same_bits(np.fromfile(str(tmp_path / ("out_" + k)), x.dtype), x), k
    # the driver
    r = subprocess.run([NODE, os.path.join(JS, "main.js"), "--tris", "20000", "--mode", "1", "--frames", "1", "--width", str(w), "--height", str(h),
                        "--dump", str(tmp_path / "d" / "BVH2.bin"), "--pick", "32,24"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    line = __import__("json").loads(r.stdout.strip().splitlines()[-1])
    big = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000, SCENE_SEED)
    gpu_ctx.set_triangles(big); gpu_ctx.build_bvh()
    _, ids, _ = orc.render(orc.make_params(w, h, 20000, cam_pos=(0, 0, 2.5), mode=orc_mod.MODE_SINGLE), big, gpu_ctx.read_bvh4(), want_tri_ids=True)
    assert line["pick"] == [32, 24] and line["prim"] == int(ids[24, 32]) and line["hit"] == (int(ids[24, 32]) != MISS)
