"""An independent float64 restatement of the build-defined path tracer and of the ray queries (section 13).

Plain numpy, vectorised over samples, brute force over every triangle: no BVH, no f16 boxes, no stack, np.sin / np.cos instead of the
polynomials.  It shares nothing with oracle/pt_oracle.cpp or the HIP kernels except the documents it was written from (and the mapping of
(u1, u2) to the local vector of the cosine-weighted direction, which DESIGN.md does not spell out).  The integer RNG is the same bits; the
rest agrees with an f32 implementation to rounding error except where a decision sits on a knife edge, and the reference says itself
which samples those are ("fragile", from margins computed here in float64, never from the code under test).

Test helper, not product code and not a conftest.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import scenes

# ---- constants of DESIGN.md section 4: the f32 values both implementations hold, widened ---------------------------------------------
F32 = np.float32
EPS_T = float(F32(1e-7))            # Moeller-Trumbore: |det| >= 1e-7, t > 1e-7
EPS_ORIGIN = float(F32(1e-4))       # so = P + nf * 1e-4
BG_PRIMARY = float(F32(0.01))
SKY = float(F32(0.15))
BASE = np.array([float(F32(0.9)), float(F32(0.7)), float(F32(0.3))])
LDIR = np.array([1.0, 1.5, 1.0]) / np.sqrt(1.0 + 2.25 + 1.0)
RR_START = 2
INF_T = 1e30                        # the finite "no hit yet" of the traversal; rays start with best = min(t_max, 1e30)

END_MISS, END_LIMIT, END_ROULETTE = 0, 1, 2
MODE_PACKET, MODE_SINGLE, MODE_PATH = 0, 1, 2

# ---- margins of the fragile flag ------------------------------------------------------------------------------------------------------
# Three to six binades above f32 rounding at unit scale (scenes stay within [-4, 4]^3).
D_B = 1e-5          # barycentrics: min(u, 1-u, v, 1-u-v) within D_B of 0
D_T = 1e-5          # t within D_T of 1e-7, of t_max, or of the closest t (a second candidate)
D_R = 1e-5          # |rnd(bounce, 4) - p|
D_N = 1e-6          # |n.d| (which side is the front), |nf.L| (NEE on / off)
D_DET = 1e-9        # ||det| - 1e-7|
D_DISC = 1e-5       # spheres: |disc| relative to hb^2 + |a cc|
# Small, distant or grazing triangles: an f32 barycentric carries an error of a few ulp times kappa = |d| e (|o| + |v0| + e) / |det|
# (e = the longer edge; the ray origin of a bounce is itself a rounded f32 position, hence |o| and not only |o - v0|).  Where
# COND_ULPS * 2^-24 * kappa exceeds the fixed margin, that is the margin.  At unit scale it does not (tetrahedron seen from 2.5: kappa = 2.5 / cos).
COND_ULPS = 16.0
U32 = 2.0 ** -24

# ---- tolerance ------------------------------------------------------------------------------------------------------------------------
# Not chosen from the code under test: this module run with dtype=float32 against its own float64 run, on every case below.  Worst
# non-fragile pixel, max_c |f32 - f64| / max(max_c |f64|, 1e-3) (numpy 2.2, x86-64; test_path_reference.py::test_tol_is_the_measured_one
# re-measures three of them and checks the arithmetic of this paragraph):
MEASURED = {
    "tetra": 1.5e-07, "soup300": 4.72e-07, "soup_inside": 3.8e-07, "room": 1.58e-07, "room_b0": 4.89e-08, "room_b1": 6.89e-08,
    "room_b2": 1.04e-07, "room_b3": 1.07e-07, "closed_box": 0.0, "back_faces": 1.23e-07, "big_triangle": 9.66e-08,
    "soup300_frame3_accum2": 6.35e-07, "room_frame2": 1.06e-07, "tetra_mode0": 2.65e-08, "tetra_mode1": 2.65e-08,
    "soup300_mode0": 6.46e-07, "soup300_mode1": 6.46e-07,
    "dragon120k": 1.59e-07, "sponza120k": 1.41e-07,   # the 120,000-triangle cases of test_gpu_path_reference.py, on their pixel subsets
    "cornell_spheres": 2.49e-05,
}
# Triangle scenes: worst 6.46e-07, x 4 = 2.6e-06, next power of ten:
TOL = 1e-5
# Spheres: the f32 discriminant cancels and the normal normalize(P - c) carries the hit point's error into n.L, so radiance is continuous
# in the rounding instead of piecewise constant.  Worst 2.49e-05, x 4 = 9.96e-05, next power of ten:
TOL_SPHERES = 1e-4

_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1)))
    return _POOL


# ---- RNG: integers, equal bits --------------------------------------------------------------------------------------------------------
def mix(x):
    """lowbias32 on uint32 arrays (wrapping arithmetic)."""
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def key(seed, pixel, sidx):
    h = mix(np.asarray(seed, np.uint32) + np.uint32(0x9E3779B9))
    h = mix(h ^ np.asarray(pixel, np.uint32))
    return mix(h ^ np.asarray(sidx, np.uint32))


def rnd(k, bounce, dim, dtype=np.float64):
    """float(mix(key ^ (bounce * 8 + dim + 1) * 0x9E3779B1) >> 8) * 2^-24: a 24-bit integer scaled by a power of two, exact in f32 and f64."""
    c = np.uint32(((bounce * 8 + dim + 1) * 0x9E3779B1) & 0xFFFFFFFF)
    h = mix(np.asarray(k, np.uint32) ^ c)
    return (h >> np.uint32(8)).astype(dtype) * dtype(U32)


# ---- scene ----------------------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, tris, spheres=None, num_tris=None, dtype=np.float64):
        T = np.asarray(tris, np.float32).reshape(-1, 3, 3)
        if num_tris is not None:
            T = T[:num_tris]
        T = T.astype(dtype)
        self.dtype = dtype
        self.v0, self.e1, self.e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
        c = np.cross(self.e1, self.e2).astype(dtype)
        with np.errstate(all="ignore"):
            self.n = (c / np.sqrt((c * c).sum(1, keepdims=True))).astype(dtype)      # geometric normal normalize(e1 x e2)
        self.m = len(T)
        self.emax = np.sqrt(np.maximum((self.e1 ** 2).sum(1), (self.e2 ** 2).sum(1)))
        self.v0n = np.sqrt((self.v0 ** 2).sum(1))
        S = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, np.float32).reshape(-1, 4)
        self.sph = S.astype(dtype)


def _rows(a):
    return a[:, 0, None], a[:, 1, None], a[:, 2, None]


def _cols(a):
    return a[None, :, 0], a[None, :, 1], a[None, :, 2]


def _dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _candidates(sc, o, d, best0):
    """Every (ray, primitive) pair: t, accepted, and the loosened / tightened acceptance the fragile flag is made of.
    Triangles in index order, then spheres.  Returns dict of (R, M + S) arrays plus u, v for the triangles."""
    dt = sc.dtype
    eps = dt(EPS_T)
    ox, oy, oz = _rows(o); dx, dy, dz = _rows(d)
    b0 = best0[:, None]
    with np.errstate(all="ignore"):
        v0x, v0y, v0z = _cols(sc.v0); e1x, e1y, e1z = _cols(sc.e1); e2x, e2y, e2z = _cols(sc.e2)
        pvx = dy * e2z - dz * e2y; pvy = dz * e2x - dx * e2z; pvz = dx * e2y - dy * e2x
        det = _dot3(e1x, e1y, e1z, pvx, pvy, pvz)
        inv = dt(1.0) / det
        sx = ox - v0x; sy = oy - v0y; sz = oz - v0z
        u = inv * _dot3(sx, sy, sz, pvx, pvy, pvz)
        qx = sy * e1z - sz * e1y; qy = sz * e1x - sx * e1z; qz = sx * e1y - sy * e1x
        v = inv * _dot3(dx, dy, dz, qx, qy, qz)
        t = inv * _dot3(e2x, e2y, e2z, qx, qy, qz)
        adet = np.abs(det)
        acc = (adet >= eps) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > eps) & (t < b0)
        # margins (float64 reasoning about an f32 implementation; meaningless, and unused, in the float32 run)
        dn = np.sqrt(_dot3(dx, dy, dz, dx, dy, dz)); on = np.sqrt(_dot3(ox, oy, oz, ox, oy, oz))
        em = sc.emax[None, :]
        kap = dn * em * (on + sc.v0n[None, :] + em) / adet
        mb = np.maximum(D_B, COND_ULPS * U32 * kap)
        mt = np.maximum(D_T, COND_ULPS * U32 * kap * em / dn)
        bary = np.minimum(np.minimum(u, 1 - u), np.minimum(v, 1 - u - v))
        loose = (adet >= eps - D_DET) & (bary > -mb) & (t > eps - mt) & (t < b0 + mt)
        tight = (adet >= eps + D_DET) & (bary >= mb) & (t >= eps + mt) & (t <= b0 - mt)
    out = dict(t=t, acc=acc, loose=loose, tight=tight, mt=mt, u=u, v=v)
    if len(sc.sph):
        with np.errstate(all="ignore"):
            cx, cy, cz = _cols(sc.sph); r = sc.sph[None, :, 3]
            ocx = ox - cx; ocy = oy - cy; ocz = oz - cz
            a = _dot3(dx, dy, dz, dx, dy, dz) + 0 * r
            hb = _dot3(ocx, ocy, ocz, dx, dy, dz)
            cc = _dot3(ocx, ocy, ocz, ocx, ocy, ocz) - r * r
            disc = hb * hb - a * cc
            sq = np.sqrt(np.maximum(disc, 0))
            t0 = (-hb - sq) / a; t1 = (-hb + sq) / a
            ts = np.where(t0 > eps, t0, t1)
            sacc = (disc >= 0) & (ts > eps) & (ts < b0)
            scale = hb * hb + np.abs(a * cc)
            # cc = oc.oc - r^2 cancels in f32 for an origin near the surface: the discriminant's error is a few ulp of hb^2 + a (oc.oc + r^2)
            err = COND_ULPS * U32 * (hb * hb + a * (cc + 2 * r * r))
            md = np.maximum(D_DISC * scale, err)
            ms = np.maximum(D_T, (err / (2 * np.maximum(sq, 1e-300)) + COND_ULPS * U32 * np.abs(hb)) / a)
            edge = (np.abs(disc) < md) | (np.abs(t0 - eps) < ms) | (np.abs(t1 - eps) < ms) | (np.abs(ts - b0) < ms)
            relevant = (t1 > eps - ms) | (np.abs(disc) < md)
            sloose = (sacc | edge) & relevant & (disc > -md) & ~(ts > b0 + ms)
            stight = sacc & ~edge
        out = dict(t=np.concatenate([t, ts], 1), acc=np.concatenate([acc, sacc], 1), loose=np.concatenate([loose, sloose], 1),
                   tight=np.concatenate([tight, stight], 1), mt=np.concatenate([mt, ms], 1), u=u, v=v)
    return out


def _closest_chunk(sc, o, d, best0):
    c = _candidates(sc, o, d, best0)
    R = len(o); ar = np.arange(R)
    tm = np.where(c["acc"], c["t"], np.inf)
    idx = np.argmin(tm, 1)                      # first minimum: index order, strict t < best
    tb = tm[ar, idx]
    hit = np.isfinite(tb)
    with np.errstate(all="ignore"):
        near = c["t"] < (tb + c["mt"][ar, idx])[:, None] + c["mt"]
        border = c["loose"] & ~c["tight"] & near
        second = c["tight"] & near
        second[ar, idx] = False
        frag = border.any(1) | second.any(1)
    m = sc.m
    tri = np.where(hit, idx, -1)
    istri = hit & (idx < m)
    ci = np.minimum(idx, m - 1) if m else idx
    u = np.where(istri, c["u"][ar, ci], 0) if m else np.zeros(R)
    v = np.where(istri, c["v"][ar, ci], 0) if m else np.zeros(R)
    return hit, tri, np.where(hit, tb, np.inf), u, v, frag


def _any_chunk(sc, o, d, best0):
    c = _candidates(sc, o, d, best0)
    occ = c["acc"].any(1)
    frag = (c["loose"] & ~c["tight"]).any(1) & ~c["tight"].any(1)      # a certain occluder settles it
    return occ, frag


def _chunked(fn, sc, o, d, best0):
    R = len(o)
    step = max(1, 160000 // max(1, sc.m + len(sc.sph)))
    parts = [(sc, o[i:i + step], d[i:i + step], best0[i:i + step]) for i in range(0, R, step)]
    if not parts:
        parts = [(sc, o, d, best0)]
    res = list(_pool().map(lambda p: fn(*p), parts)) if len(parts) > 1 else [fn(*parts[0])]
    return [np.concatenate([r[k] for r in res]) for k in range(len(res[0]))]


def closest_hit(sc, o, d, t_max=None):
    """-> hit, prim (-1 on a miss; spheres as m + i), t, u, v, fragile."""
    o = np.asarray(o, sc.dtype).reshape(-1, 3); d = np.asarray(d, sc.dtype).reshape(-1, 3)
    best0 = np.full(len(o), INF_T, sc.dtype) if t_max is None else np.minimum(np.asarray(t_max, sc.dtype), sc.dtype(INF_T))
    return _chunked(_closest_chunk, sc, o, d, best0)


def any_hit(sc, o, d, t_max=None):
    """-> occluded (an accepted primitive exists), fragile."""
    o = np.asarray(o, sc.dtype).reshape(-1, 3); d = np.asarray(d, sc.dtype).reshape(-1, 3)
    best0 = np.full(len(o), INF_T, sc.dtype) if t_max is None else np.minimum(np.asarray(t_max, sc.dtype), sc.dtype(INF_T))
    return _chunked(_any_chunk, sc, o, d, best0)


def _query_chunk(sc, o, d, best0):
    c = _candidates(sc, o, d, best0)
    R = len(o); ar = np.arange(R)
    tm = np.where(c["acc"], c["t"], np.inf)
    idx = np.argmin(tm, 1)
    tb = tm[ar, idx]
    hit = np.isfinite(tb)
    with np.errstate(all="ignore"):
        near = c["t"] < (tb + c["mt"][ar, idx])[:, None] + c["mt"]
        border = c["loose"] & ~c["tight"]
        second = c["tight"] & near
        second[ar, idx] = False
        frag = (border & near).any(1) | second.any(1)
        afrag = border.any(1) & ~c["tight"].any(1)
    t_sure = np.where(c["tight"], c["t"], np.inf).min(1)         # the closest triangle accepted with every margin to spare
    return hit, np.where(hit, idx, -1), np.where(hit, tb, np.inf), np.where(hit, c["u"][ar, idx], 0), np.where(hit, c["v"][ar, idx], 0), frag, c["acc"].any(1), afrag, t_sure


def query(tris, O, D, t_max=None, dtype=np.float64):
    """Ray queries by brute force: -> dict(hit, prim, t, u, v, fragile, any, any_fragile, t_sure).  Rays start with
    best = min(t_max, 1e30); triangles only (spheres take no part in queries)."""
    sc = Scene(tris, dtype=dtype)
    o = np.asarray(O, np.float32).astype(dtype).reshape(-1, 3); d = np.asarray(D, np.float32).astype(dtype).reshape(-1, 3)
    best0 = np.full(len(o), INF_T, dtype) if t_max is None else np.minimum(np.asarray(t_max, np.float32).astype(dtype), dtype(INF_T))
    r = _chunked(_query_chunk, sc, o, d, best0)
    return dict(zip(("hit", "prim", "t", "u", "v", "fragile", "any", "any_fragile", "t_sure"), r))


def pair(tris, O, D, prim, dtype=np.float64):
    """Moeller-Trumbore of ray i against triangle prim[i] alone: -> det, u, v, t."""
    dt = dtype
    T = np.asarray(tris, np.float32).reshape(-1, 3, 3).astype(dt)[np.asarray(prim, np.int64)]
    o = np.asarray(O, np.float32).astype(dt); d = np.asarray(D, np.float32).astype(dt)
    v0, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    pv = cross(d, e2); det = dot(e1, pv)
    with np.errstate(all="ignore"):
        inv = dt(1) / det; s = o - v0
        u = inv * dot(s, pv); q = cross(s, e1); v = inv * dot(d, q); t = inv * dot(e2, q)
    return det, u, v, t


def loosely_accepts(tris, O, D, prim, t_max=None):
    """Could an f32 implementation accept triangle prim[i] for ray i?  (Accepted with every margin of the fragile flag in its favour.)
    For results that depend on the visit order -- any-hit's prim -- and for fragile rays.  -> (bool, that pair's float64 t)."""
    sc = Scene(np.asarray(tris, np.float32).reshape(-1, 9)[np.asarray(prim, np.int64)])
    o = np.asarray(O, np.float32).astype(np.float64); d = np.asarray(D, np.float32).astype(np.float64)
    best0 = np.full(len(o), INF_T) if t_max is None else np.minimum(np.asarray(t_max, np.float32).astype(np.float64), INF_T)
    ok = np.zeros(len(o), bool); t = np.zeros(len(o))
    for i in range(0, len(o), 256):                     # (R, R) candidate blocks; the diagonal is ray i against its own triangle
        sub = Scene.__new__(Scene)
        j = slice(i, i + 256)
        sub.dtype = np.float64; sub.sph = np.zeros((0, 4))
        sub.v0, sub.e1, sub.e2, sub.emax, sub.v0n = sc.v0[j], sc.e1[j], sc.e2[j], sc.emax[j], sc.v0n[j]
        c = _candidates(sub, o[j], d[j], best0[j])
        ok[j] = np.diag(c["loose"] | c["acc"]); t[j] = np.diag(c["t"])
    return ok, t


# ---- camera ---------------------------------------------------------------------------------------------------------------------------
def focal_aspect(width, height):
    """fov 70 degrees, computed in double, stored as f32: the values a caller passes."""
    fov = (70.0 * np.pi) / 180
    return np.float32(1.0 / np.tan(0.5 * fov)), np.float32(width / height)


def _normalize(v):
    return v / np.sqrt((v * v).sum(1, keepdims=True))


def camera_rays(fx, fy, width, height, focal, aspect, cam_pos, cam_quat, dtype=np.float64):
    dt = dtype
    x = (fx / dt(width)) * dt(2) - dt(1); y = (fy / dt(height)) * dt(2) - dt(1)
    d = _normalize(np.stack([x * dt(aspect), y, np.full_like(x, -dt(focal))], 1))
    q = np.asarray(cam_quat, np.float32).astype(dt)
    uq = np.broadcast_to(q[:3], d.shape); s = q[3]
    uv = np.cross(uq, d).astype(dt); uuv = np.cross(uq, uv).astype(dt)
    d = d + dt(2) * (s * uv + uuv)
    o = np.broadcast_to(np.asarray(cam_pos, np.float32).astype(dt), d.shape).copy()
    return o, d.astype(dt)


def cosine_dir(n, u1, u2):
    """Cosine-weighted direction around n: local (sqrt(u1) cos 2 pi u2, sqrt(u1) sin 2 pi u2, sqrt(1 - u1)) in the basis of Duff et al. 2017."""
    dt = n.dtype.type
    ang = dt(2 * np.pi) * u2
    r = np.sqrt(u1)
    lx, ly, lz = r * np.cos(ang), r * np.sin(ang), np.sqrt(dt(1) - u1)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sg = np.copysign(dt(1), nz)
    a = dt(-1) / (sg + nz)
    b = nx * ny * a
    t = np.stack([dt(1) + sg * nx * nx * a, sg * b, -sg * nx], 1)
    bt = np.stack([b, sg + ny * ny * a, -ny], 1)
    return t * lx[:, None] + bt * ly[:, None] + n * lz[:, None]


# ---- the renderer ---------------------------------------------------------------------------------------------------------------------
class Result:
    """img: (H, W, 3), or (K, 3) with `pixels`.  fragile: per pixel.  Per sample, shape (pixels, frames * spp): frag, length (closest rays traced),
    end (END_*), shadow_clear / shadow_occluded (counts), primary_tri (-1 on a miss), primary_back.  Totals: rays_closest, rays_shadow, samples."""


def render(tris, width, height, cam_pos=(0, 0, 2.5), cam_quat=(0, 0, 0, 1), mode=MODE_PATH, spp=1, max_bounces=0, seed=1, frame=0,
           accum_frames=1, spheres=None, num_tris=None, pixels=None, roulette=True, dtype=np.float64, focal=None, aspect=None):
    dt = dtype
    sc = Scene(tris, spheres, num_tris, dt)
    if focal is None:
        focal, aspect = focal_aspect(width, height)
    if pixels is None:
        py, px = np.divmod(np.arange(width * height), width)
    else:
        pixels = np.asarray(pixels).reshape(-1, 2)
        px, py = pixels[:, 0], pixels[:, 1]
    K = len(px)
    base = BASE.astype(dt); L = LDIR.astype(dt)
    res = Result()
    if mode != MODE_PATH:
        o, d = camera_rays(px.astype(dt) + dt(0.5), py.astype(dt) + dt(0.5), width, height, focal, aspect, cam_pos, cam_quat, dt)
        hit, tri, t, _, _, frag = closest_hit(sc, o, d)
        n = _hit_normals(sc, tri, hit, o, d, t)
        ndl = np.maximum((n * L).sum(1), dt(0))                    # n, not nf: the reference's shade()
        img = np.where(hit[:, None], base[None, :] * (dt(SKY) + ndl)[:, None], dt(BG_PRIMARY))
        res.fragile = frag; res.frag = frag[:, None]; res.primary_tri = tri[:, None]
        res.rays_closest = K; res.rays_shadow = 0; res.samples = K
        res.img = img if pixels is not None else img.reshape(height, width, 3)
        if pixels is None:
            res.fragile = frag.reshape(height, width)
        return res

    S = accum_frames * spp
    N = K * S
    pix_of = np.repeat(np.arange(K), S)
    sidx = np.tile((frame * spp + np.arange(S)).astype(np.uint32), K)          # sidx = f * spp + s over consecutive frames
    k = key(np.uint32(seed), (py.astype(np.uint32) * np.uint32(width) + px.astype(np.uint32))[pix_of], sidx)
    fx = px[pix_of].astype(dt) + rnd(k, 0, 0, dt); fy = py[pix_of].astype(dt) + rnd(k, 0, 1, dt)
    o, d = camera_rays(fx, fy, width, height, focal, aspect, cam_pos, cam_quat, dt)
    rad = np.zeros((N, 3), dt); T = np.ones((N, 3), dt)
    frag = np.zeros(N, bool); length = np.zeros(N, np.int32); end = np.full(N, -1, np.int32)
    sh_clear = np.zeros(N, np.int32); sh_occ = np.zeros(N, np.int32)
    ptri = np.full(N, -1, np.int64); pback = np.zeros(N, bool)
    act = np.arange(N)
    bounce = 0
    while len(act):
        hit, tri, t, _, _, fr = closest_hit(sc, o, d)
        length[act] += 1; frag[act] |= fr
        miss = act[~hit]
        rad[miss] += T[miss] * dt(BG_PRIMARY if bounce == 0 else SKY); end[miss] = END_MISS
        act, o, d, t, tri = act[hit], o[hit], d[hit], t[hit], tri[hit]
        if not len(act):
            break
        n = _hit_normals(sc, tri, np.ones(len(act), bool), o, d, t)
        P = o + d * t[:, None]
        nd = (n * d).sum(1)
        frag[act] |= np.abs(nd) < D_N
        front = nd < 0
        nf = np.where(front[:, None], n, -n)
        if bounce == 0:
            ptri[act] = tri; pback[act] = ~front
        so = P + nf * dt(EPS_ORIGIN)
        ndl = (nf * L).sum(1)
        frag[act] |= np.abs(ndl) < D_N
        lit = ndl > 0
        if lit.any():
            occ, fr = any_hit(sc, so[lit], np.broadcast_to(L, (int(lit.sum()), 3)))
            la = act[lit]
            frag[la] |= fr
            sh_occ[la] += occ; sh_clear[la] += ~occ
            c = la[~occ]
            rad[c] += (T[c] * base) * ndl[lit][~occ][:, None]
        if bounce >= max_bounces:
            end[act] = END_LIMIT
            break
        T[act] *= base
        go = np.ones(len(act), bool)
        if roulette and bounce >= RR_START:
            p = T[act].max(1)
            r = rnd(k[act], bounce, 4, dt)
            frag[act] |= np.abs(r - p) < D_R
            go = ~(r >= p)
            end[act[~go]] = END_ROULETTE
            T[act[go]] /= p[go][:, None]
        d = cosine_dir(nf[go], rnd(k[act[go]], bounce, 2, dt), rnd(k[act[go]], bounce, 3, dt))
        o = so[go]; act = act[go]
        bounce += 1
    img = rad.reshape(K, S, 3).sum(1) / dt(S)
    res.frag = frag.reshape(K, S); res.length = length.reshape(K, S); res.end = end.reshape(K, S)
    res.shadow_clear = sh_clear.reshape(K, S); res.shadow_occluded = sh_occ.reshape(K, S)
    res.primary_tri = ptri.reshape(K, S); res.primary_back = pback.reshape(K, S)
    res.sample_rad = rad.reshape(K, S, 3)
    res.rays_closest = int(length.sum()); res.rays_shadow = int(sh_clear.sum() + sh_occ.sum()); res.samples = N
    res.fragile = res.frag.any(1)
    res.img = img
    if pixels is None:
        res.img = img.reshape(height, width, 3); res.fragile = res.fragile.reshape(height, width)
    return res


def _hit_normals(sc, tri, hit, o, d, t):
    dt = sc.dtype
    n = np.zeros((len(tri), 3), dt)
    istri = hit & (tri < sc.m) & (tri >= 0)
    n[istri] = sc.n[tri[istri]]
    iss = hit & (tri >= sc.m)
    if iss.any():
        c = sc.sph[tri[iss] - sc.m, :3]
        n[iss] = _normalize((o[iss] + d[iss] * t[iss][:, None]) - c)
    return n


# ---- comparison -----------------------------------------------------------------------------------------------------------------------
def deviation(got, ref):
    """Per pixel: max_c |got - ref| / max(max_c |ref|, 1e-3)."""
    got = np.asarray(got, np.float64)[..., :3]; ref = np.asarray(ref, np.float64)[..., :3]
    return np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-3)


FRAGILE_CAP = 0.02


def check_image(got, ref, tol, name=""):
    """Every non-fragile pixel within tol; fragile pixels are not compared and are at most 2 % of the case.  Returns the worst deviation."""
    dev = deviation(got, ref.img)
    fr = ref.fragile
    share = float(fr.mean())
    worst = float(dev[~fr].max()) if (~fr).any() else 0.0
    print("%s: fragile %.3f %% of %d pixels, worst non-fragile deviation %.3g, fragile pixels off %d" % (name, 100 * share, fr.size, worst, int((dev[fr] > tol).sum())))
    assert share <= FRAGILE_CAP, "%s: %.2f %% of the pixels are fragile (cap 2 %%): badly chosen geometry" % (name, 100 * share)
    bad = np.argwhere((dev > tol) & ~fr)
    assert len(bad) == 0, "%s: %d non-fragile pixels off by more than %g (worst %.3g, first at %s); %d fragile pixels differ too" % (
        name, len(bad), tol, worst, bad[:5].tolist(), int((dev[fr] > tol).sum()))
    return worst


# ---- the cases both test files run ----------------------------------------------------------------------------------------------------
def _quat(yaw, pitch):
    return tuple(float(x) for x in scenes.quat_yaw_pitch(yaw, pitch))


def case(name):
    """-> (tris, spheres or None, width, height, render keywords)."""
    kw = dict(mode=MODE_PATH, spp=4, max_bounces=8, seed=7)
    if name == "tetra":
        return scenes.TETRA, None, 96, 64, kw
    if name == "soup300":
        return scenes.random_soup(300, 3, size=0.5), None, 96, 64, kw
    if name == "soup_inside":
        return scenes.random_soup(500, 5, size=0.25), None, 64, 48, dict(kw, cam_pos=(0.03, -0.02, 0.05))
    if name == "room":
        return scenes.room(), None, 96, 64, dict(kw, cam_pos=(0.0, 0.0, 0.95))
    if name.startswith("room_b"):                         # max_bounces 0, 1, 2, 3: the roulette threshold sits between 2 and 3
        return scenes.room(), None, 48, 32, dict(kw, cam_pos=(0.0, 0.0, 0.95), max_bounces=int(name[6:]))
    if name == "closed_box":
        return scenes.closed_box(), None, 64, 48, dict(kw, cam_pos=(0.1, 0.05, 0.2))
    if name == "back_faces":
        return scenes.back_faces(), None, 64, 48, kw
    if name == "big_triangle":
        return scenes.BIG_TRIANGLE, None, 64, 48, dict(kw, max_bounces=2)
    if name == "cornell_spheres":
        t, s = scenes.cornell()
        return t, s, 64, 64, dict(kw, max_bounces=3)
    if name == "soup300_frame3_accum2":                   # frame > 0, two frames accumulated, another seed, odd non-square size, turned camera
        return scenes.random_soup(300, 3, size=0.5), None, 75, 41, dict(kw, spp=2, seed=11, frame=3, accum_frames=2, cam_pos=(1.2, 0.8, 2.2), cam_quat=_quat(0.5, -0.3))
    if name == "room_frame2":
        return scenes.room(), None, 53, 37, dict(kw, spp=2, seed=11, frame=2, cam_pos=(0.2, -0.1, 0.9), cam_quat=_quat(-0.25, 0.15))
    if name in ("tetra_mode0", "tetra_mode1"):
        return scenes.TETRA, None, 96, 64, dict(mode=int(name[-1]))
    if name in ("soup300_mode0", "soup300_mode1"):
        return scenes.random_soup(300, 3, size=0.5), None, 75, 41, dict(mode=int(name[-1]), cam_pos=(1.2, 0.8, 2.2), cam_quat=_quat(0.5, -0.3))
    raise KeyError(name)


PATH_CASES = ["tetra", "soup300", "soup_inside", "room", "room_b0", "room_b1", "room_b2", "room_b3", "closed_box", "back_faces", "big_triangle",
              "soup300_frame3_accum2", "room_frame2"]
MODE01_CASES = ["tetra_mode0", "tetra_mode1", "soup300_mode0", "soup300_mode1"]
SPHERE_CASES = ["cornell_spheres"]

_CACHE = {}


def reference(name, **override):
    """The float64 reference of a case (cached per process: both the oracle's and the kernels' tests of a case use one run)."""
    k = (name, tuple(sorted(override.items())))
    if k not in _CACHE:
        tris, sph, w, h, kw = case(name)
        _CACHE[k] = render(tris, w, h, spheres=sph, **dict(kw, **override))
    return _CACHE[k]
