"""csrc/pt_cut.h restated in numpy float32, operation for operation (include/mi355pt.h pt_cut_search), with the
float64 margin of the plane test and exact rationals for the exact cases.  Every array operation below is one f32 operation per element,
in the order of the header; numpy never fuses a multiply with an add."""
from fractions import Fraction

import numpy as np

f32 = np.float32


def walked(rec):
    """the records that are walked: n and d finite, n not the zero vector, the window finite with lo <= hi"""
    r = np.asarray(rec, f32)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(r[:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]]).all(1) & (r[:, 0:3] != 0).any(1) & (r[:, 4:7] <= r[:, 8:11]).all(1))


def records(tris, ti):
    """v0, e1, e2 of the triangle records (csrc/pt_host.cpp::build_tri_records): the edges are f32 differences of the vertices"""
    T = np.asarray(tris, f32).reshape(-1, 3, 3)[np.asarray(ti, np.int64)]
    return T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]


def side(r, v):
    """ptct::side of the (m, 3) f32 points v for the (m, 12) records r: ((n.x*x + n.y*y) + n.z*z) - d"""
    s = ((r[:, 0] * v[:, 0] + r[:, 1] * v[:, 1]) + r[:, 2] * v[:, 2]) - r[:, 3]
    assert s.dtype == f32
    return s


def box_stage(r, v0, v1, v2):
    """pttt::box_stage: the three record vertices against the window as given"""
    lo, hi = r[:, 4:7], r[:, 8:11]
    le = [v <= hi for v in (v0, v1, v2)]
    ge = [v >= lo for v in (v0, v1, v2)]
    return ((le[0] | le[1] | le[2]) & (ge[0] | ge[1] | ge[2]) & (le[0] | ge[0]) & (le[1] | ge[1]) & (le[2] | ge[2])).all(1)


def cross_t(si, sj):
    """ptct::cross_t: s_a / (s_a - s_b), a the end below the plane"""
    below = si < 0
    sa, sb = np.where(below, si, sj), np.where(below, sj, si)
    return sa / (sa - sb)


def tri_cut(rec, tris, pi, ti):
    """ptct::tri_cut<true> for the pairs (pi[j], ti[j]): -> (accepted, code, t0, t1); code, t0, t1 mean something where accepted"""
    r = np.asarray(rec, f32)[np.asarray(pi, np.int64)]
    v0, e1, e2 = records(tris, ti)
    with np.errstate(all="ignore"):
        v1, v2 = v0 + e1, v0 + e2
        a = box_stage(r, v0, v1, v2)
        s0, s1, s2 = side(r, v0), side(r, v1), side(r, v2)
        u0, u1, u2 = s0 >= 0, s1 >= 0, s2 >= 0
        l0, l1, l2 = s0 < 0, s1 < 0, s2 < 0
        b = (u0 | l0) & (u1 | l1) & (u2 | l2) & (u0 | u1 | u2) & (l0 | l1 | l2)
        c01, c12, c02 = u0 != u1, u1 != u2, u0 != u2
        code = (c01 * 1 + c12 * 2 + c02 * 4 + u0 * 8 + u1 * 16 + u2 * 32).astype(np.uint32)
        t12 = cross_t(s1, s2)
        t0 = np.where(c01, cross_t(s0, s1), t12)
        t1 = np.where(c02, cross_t(s0, s2), t12)
    assert t0.dtype == f32 and t1.dtype == f32
    return a & b, code, t0, t1


def numpy_brute(rec, tris, chunk_pairs=1 << 21):
    """The brute-force list restated: every triangle in index order through tri_cut.  Returns (offsets, prim, code, t0, t1)."""
    r = np.asarray(rec, f32)
    n, m = len(r), np.asarray(tris).size // 9
    ok = walked(r)
    counts = np.zeros(n, np.int64)
    parts = [[], [], [], []]
    step = max(1, chunk_pairs // max(m, 1))
    for s in range(0, n, step):
        sel = np.arange(s, min(s + step, n))
        sel = sel[ok[sel]]
        if not len(sel) or not m:
            continue
        pi = np.repeat(sel, m); ti = np.tile(np.arange(m), len(sel))
        acc, code, t0, t1 = tri_cut(r, tris, pi, ti)
        counts += np.bincount(pi[acc], minlength=n)
        for p, x in zip(parts, (ti[acc].astype(np.uint32), code[acc], t0[acc], t1[acc])):
            p.append(x)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    cat = lambda p, dt: np.concatenate(p) if p else np.zeros(0, dt)
    return offsets, cat(parts[0], np.uint32), cat(parts[1], np.uint32), cat(parts[2], f32), cat(parts[3], f32)


def node_cut(rec, mn, mx):
    """ptct::node_cut of record rec (12 f32) on the decoded child boxes mn, mx ((k, 3) f32 each) -> (k,) bool"""
    r = np.broadcast_to(np.asarray(rec, f32), (len(mn), 12))
    s = f32(2.0 ** -12)
    with np.errstate(all="ignore"):
        gl, gh = np.asarray(mn, f32) - s, np.asarray(mx, f32) + s
        up = r[:, 0:3] >= 0
        sp, sn = side(r, np.where(up, gh, gl)), side(r, np.where(up, gl, gh))
        return (sp >= 0) & (sn < 0)


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------
def sides64(rec, tris, pi, ti):
    """s_i of the pairs in float64, from the f32 plane and the f32 vertices themselves: (m, 3)"""
    r = np.asarray(rec, f32).astype(np.float64)[np.asarray(pi, np.int64)]
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)[np.asarray(ti, np.int64)]
    return np.einsum("nic,nc->ni", T, r[:, 0:3]) - r[:, 3:4]


def margin64(rec, tris, pi, ti):
    """G of the pairs: +min_i |s_i| where the triangle straddles the plane in float64 (some s_i >= 0 and some s_i < 0), -min_i |s_i|
    where it does not"""
    s = sides64(rec, tris, pi, ti)
    straddles = (s >= 0).any(1) & (s < 0).any(1)
    return np.where(straddles, 1.0, -1.0) * np.abs(s).min(1)


# ---- exact rationals ----------------------------------------------------------------------------------------------------------------------
def cut_exact(normal, d, tri):
    """The leaf test (b) on exact rationals for one plane and one triangle (9 numbers): None where not accepted, else (code, t0, t1) with
    t0, t1 Fractions."""
    n = [Fraction(float(x)) for x in normal]
    v = [[Fraction(float(x)) for x in np.asarray(tri, np.float64).reshape(3, 3)[i]] for i in range(3)]
    s = [sum(a * b for a, b in zip(n, v[i])) - Fraction(float(d)) for i in range(3)]
    u = [x >= 0 for x in s]
    if all(u) or not any(u):
        return None
    edges = [(0, 1), (1, 2), (0, 2)]
    cross = [u[i] != u[j] for i, j in edges]
    code = sum(1 << k for k in range(3) if cross[k]) | sum(8 << i for i in range(3) if u[i])

    def t(k):
        i, j = edges[k]
        a, b = (i, j) if s[i] < 0 else (j, i)
        return s[a] / (s[a] - s[b])
    ks = [k for k in range(3) if cross[k]]
    return code, t(ks[0]), t(ks[-1])
