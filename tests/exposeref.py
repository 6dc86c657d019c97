"""Exposed triangles restated in numpy float64, without the package: every pair of triangles, no tree.

A triangle T is exposed when no triangle N of the scene (T and its neighbours included) has a point x with
  * the projection of x along the light inside the projection of T' pushed out by rho_xy + rho_n + rho_N, T' = T shifted by 1e-4 along its
    unit normal on the light's side, and
  * the height of x over the plane of T', measured along the light, above -(rho_n + rho_N) / c, c = |n . L|,
where rho_n, rho_xy bound how far a shadow-ray origin of the kernel can lie off the plane of T' and off T' inside that plane, and
rho_N = kappa_N * S bounds how far from N an accepted Moller-Trumbore test of N can be.

`slack` moves every threshold by that much towards "blocked" (positive) or "free" (negative): the band the device's mask has to lie in.
`rho_scale` and `shift` exist so that the tests can show a wrong definition failing (rho_scale = -1: margins negated; shift = 0: no shift)."""
import numpy as np

EPS32 = 2.0 ** -24
SHIFT = 1e-4
C_MIN = 0.02
GATE = 0.0999
NORMAL_TOL = 1e-5
DET_MIN = 9.99e-8


def light32():
    """the kernel's light direction, f32: normalize(1, 1.5, 1) as v * (1 / sqrt(dot))"""
    v = np.array([1.0, 1.5, 1.0], np.float32)
    d = np.float32(np.float32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    inv = np.float32(1.0) / np.sqrt(d, dtype=np.float32)
    return (v * inv).astype(np.float32)


def records(tris):
    """(v0, e1, e2, n32) as the arena holds them: edges and normal computed in f32"""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    v0 = t[:, 0]; e1 = (t[:, 1] - t[:, 0]).astype(np.float32); e2 = (t[:, 2] - t[:, 0]).astype(np.float32)
    cx = (e1[:, 1] * e2[:, 2]).astype(np.float32) - (e1[:, 2] * e2[:, 1]).astype(np.float32)
    cy = (e1[:, 2] * e2[:, 0]).astype(np.float32) - (e1[:, 0] * e2[:, 2]).astype(np.float32)
    cz = (e1[:, 0] * e2[:, 1]).astype(np.float32) - (e1[:, 1] * e2[:, 0]).astype(np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / np.sqrt(((cx * cx).astype(np.float32) + (cy * cy).astype(np.float32)).astype(np.float32) + (cz * cz).astype(np.float32), dtype=np.float32)
        n32 = np.stack([cx * inv, cy * inv, cz * inv], 1).astype(np.float32)
    return v0.astype(np.float64), e1.astype(np.float64), e2.astype(np.float64), n32


def basis():
    L = light32().astype(np.float64)
    Lh = L / np.linalg.norm(L)
    U = np.cross(Lh, [1.0, 0.0, 0.0]); U /= np.linalg.norm(U)
    V = np.cross(Lh, U)
    return L, Lh, U, V


def _clip(poly, a, b, d):
    """Sutherland-Hodgman: the part of the polygon (rows u, v, h) with a u + b v + d >= 0"""
    out = []
    m = len(poly)
    for i in range(m):
        p, q = poly[i], poly[(i + 1) % m]
        sp, sq = a * p[0] + b * p[1] + d, a * q[0] + b * q[1] + d
        if sp >= 0.0:
            out.append(p)
        if (sp >= 0.0) != (sq >= 0.0):
            f = sp / (sp - sq)
            out.append(p + f * (q - p))
    return out


def flags(tris, s_max, d_max, slack=0.0, rho_scale=1.0, shift=SHIFT, detail=False):
    v0, e1, e2, n32 = records(tris)
    n = len(v0)
    L, Lh, U, V = basis()
    with np.errstate(all="ignore"):
        nn = np.cross(e1, e2); a2 = np.linalg.norm(nn, axis=1)
        l1 = np.linalg.norm(e1, axis=1); l2 = np.linalg.norm(e2, axis=1)
        nh = nn / a2[:, None]
        sinphi = a2 / (l1 * l2)
        det = np.abs(np.einsum("ij,ij->i", e1, np.cross(L[None, :], e2)))
        can_accept = det + 5.3 * EPS32 * l1 * l2 >= DET_MIN - slack * 1e-3
        kappa = 36.0 * EPS32 * l1 * l2 / det
        cl = nh @ Lh
        c = np.abs(cl)
        rho_n = (EPS32 * (11.5 * s_max / sinphi + 3.0 * s_max + 7.0 * d_max) + 2e-9) * rho_scale
        rho_xy = (36.0 * EPS32 * s_max / (sinphi * GATE)) * rho_scale + rho_n
        ok = (a2 > 0) & np.isfinite(a2) & (np.linalg.norm(nh - n32, axis=1) <= NORMAL_TOL - slack) & (c >= C_MIN + slack) & (np.abs(rho_n) < SHIFT - slack)
    verts = np.stack([v0, v0 + e1, v0 + e2], 1)                        # n x 3 x 3
    pu, pv = verts @ U, verts @ V                                      # n x 3
    out = np.zeros(n, bool)
    for t in np.nonzero(ok)[0]:
        nf = nh[t] * (1.0 if cl[t] >= 0 else -1.0)
        ts = verts[t] + shift * nf
        tp = np.stack([ts @ U, ts @ V], 1)
        area = (tp[1, 0] - tp[0, 0]) * (tp[2, 1] - tp[0, 1]) - (tp[1, 1] - tp[0, 1]) * (tp[2, 0] - tp[0, 0])
        if area == 0.0:
            continue
        o = 1.0 if area > 0 else -1.0
        cen = ts.mean(0); rad = np.linalg.norm(ts - cen, axis=1).max()
        with np.errstate(all="ignore"):
            S = np.linalg.norm(v0 - cen, axis=1) + rad + rho_xy[t] + l1 + l2
            rho_nb = kappa * S * rho_scale
            grow = rho_xy[t] + rho_n[t] + rho_nb + slack
            hthr = -(rho_n[t] + rho_nb + slack) / c[t]
            h = ((verts - ts[0]) @ nf) / c[t]                          # n x 3 heights over the shifted plane along the light
        cand = can_accept & ~(grow < np.inf)
        near = can_accept & (pu.min(1) <= tp[:, 0].max() + grow) & (pu.max(1) >= tp[:, 0].min() - grow) & \
            (pv.min(1) <= tp[:, 1].max() + grow) & (pv.max(1) >= tp[:, 1].min() - grow) & (h.max(1) > hthr)
        blocked = bool(cand.any())
        for k in np.nonzero(near)[0]:
            if blocked:
                break
            poly = [np.array([pu[k, i], pv[k, i], h[k, i]]) for i in range(3)]
            for i in range(3):
                a_, c_ = tp[i], tp[(i + 1) % 3]
                ex, ey = c_[0] - a_[0], c_[1] - a_[1]
                il = 1.0 / np.hypot(ex, ey)
                na, nb = -ey * il * o, ex * il * o
                poly = _clip(poly, na, nb, -(na * a_[0] + nb * a_[1]) + grow[k])
                if not poly:
                    break
            blocked = any(p[2] > hthr[k] for p in poly)
        out[t] = not blocked
    if detail:
        return out, {"ok": ok, "c": c, "cl": cl, "nh": nh, "rho_n": rho_n, "rho_xy": rho_xy}
    return out
