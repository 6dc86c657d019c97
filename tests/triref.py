"""Three restatements of the triangle-overlap test (include/mi355pt.h pt_tri_search, csrc/pt_tritri.h), none of them
the twin: a numpy float32 one, operation for operation; a float64 reference with a margin in units of length; and an exact-rational one
(fractions.Fraction) for lattice inputs, which gives the expected `edges` of the exact cases.

A pair is (caller triangle q0, q1, q2; mesh triangle record v0, e1 = v1 - v0, e2 = v2 - v0).  Its six segment tests, in the order of the
bits of `edges`: the caller's edges (q0, q1 - q0), (q1, q2 - q1), (q2, q0 - q2) against (v0, e1, e2), then the mesh edges (v0, e1),
(v0 + e1, e2 - e1), (v0, e2) against (q0, q1 - q0, q2 - q0)."""
from fractions import Fraction

import numpy as np

f32 = np.float32


def records(tris, ti):
    """v0, e1, e2 of the triangle records (csrc/pt_host.cpp::build_tri_records): the edges are f32 differences of the vertices"""
    T = np.asarray(tris, f32).reshape(-1, 3, 3)[np.asarray(ti, np.int64)]
    return T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]


def callers(rec):
    """(n, 12) PtTri records -> (n, 3, 3) vertices"""
    return np.asarray(rec, f32).reshape(-1, 3, 4)[:, :, :3]


def walked(rec):
    return np.isfinite(callers(rec)).all((1, 2))


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def six_tests(Q, v0, e1, e2):
    """[(p, d, a, f1, f2)] of the six segment tests, every difference and sum in the dtype of the inputs"""
    q0, q1, q2 = Q[:, 0], Q[:, 1], Q[:, 2]
    a, c = q1 - q0, q2 - q0
    return [(q0, a, v0, e1, e2), (q1, q2 - q1, v0, e1, e2), (q2, q0 - q2, v0, e1, e2),
            (v0, e1, q0, a, c), (v0 + e1, e2 - e1, q0, a, c), (v0, e2, q0, a, c)]


# ---- csrc/pt_tritri.h restated in numpy float32, operation for operation ------------------------------------------------------------
def seg_crosses32(p, d, a, f1, f2):
    assert all(x.dtype == f32 for x in (p, d, a, f1, f2))
    with np.errstate(all="ignore"):
        pv = _cross(d, f2)
        det = _dot(f1, pv)
        sv = p - a
        U = _dot(sv, pv)
        qv = _cross(sv, f1)
        V = _dot(d, qv)
        T = _dot(f2, qv)
        W = U + V
        pos = (det > 0) & (U >= 0) & (V >= 0) & (W <= det) & (T >= 0) & (T <= det)
        neg = (det < 0) & (U <= 0) & (V <= 0) & (W >= det) & (T <= 0) & (T >= det)
    assert det.dtype == f32 and W.dtype == f32
    return pos | neg


def box_stage32(rec, tris, ci, ti):
    """(a): the record's three vertices against the caller triangle's exact bounding box"""
    Q = callers(rec)[ci]
    lo, hi = Q.min(1), Q.max(1)
    v0, e1, e2 = records(tris, ti)
    with np.errstate(all="ignore"):
        v1, v2 = v0 + e1, v0 + e2
        le = [v <= hi for v in (v0, v1, v2)]
        ge = [v >= lo for v in (v0, v1, v2)]
    return ((le[0] | le[1] | le[2]) & (ge[0] | ge[1] | ge[2]) & (le[0] | ge[0]) & (le[1] | ge[1]) & (le[2] | ge[2])).all(1)


def edges32(rec, tris, ci, ti):
    """the `edges` word of the pairs (ci[j], ti[j]), the box stage not applied"""
    v0, e1, e2 = records(tris, ti)
    out = np.zeros(len(ci), np.uint32)
    for bit, t in enumerate(six_tests(callers(rec)[ci], v0, e1, e2)):
        out |= seg_crosses32(*t).astype(np.uint32) << np.uint32(bit)
    return out


def numpy_brute(rec, tris, chunk_pairs=1 << 21):
    """The brute-force list restated in numpy float32: every mesh triangle in index order, (a) on every pair of a walked caller triangle,
    the six segment tests on the pairs that pass it.  Returns (offsets, prim, edges)."""
    rec = np.asarray(rec, f32)
    n, m = len(rec), np.asarray(tris).size // 9
    ok = walked(rec)
    counts = np.zeros(n, np.int64)
    prims, words = [], []
    step = max(1, chunk_pairs // max(m, 1))
    for s in range(0, n, step):
        sel = np.arange(s, min(s + step, n))
        sel = sel[ok[sel]]
        if not len(sel) or not m:
            continue
        ci = np.repeat(sel, m); ti = np.tile(np.arange(m), len(sel))
        a = box_stage32(rec, tris, ci, ti)
        ci, ti = ci[a], ti[a]
        e = edges32(rec, tris, ci, ti)
        acc = e != 0
        counts += np.bincount(ci[acc], minlength=n)
        prims.append(ti[acc].astype(np.uint32)); words.append(e[acc])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return offsets, cat(prims), cat(words)


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------
def seg_margin64(p, d, a, f1, f2):
    """The margin of one segment-triangle test in units of length, the minimum of
      the plane margin: min(|h_p|, |h_q|) of the end points' signed distances to the triangle's plane, positive iff they lie on opposite
        sides or on it;
      three side margins: s U / (|d| |f2|), s V / (|d| |f1|), s (det - U - V) / (|d| |f2 - f1|) with s = sign(det).
    A test whose det, normal or segment is zero crosses nothing: -inf."""
    n = np.cross(f1, f2)
    nn = np.linalg.norm(n, axis=1)
    pv = np.cross(d, f2)
    det = np.einsum("ij,ij->i", f1, pv)
    sv = p - a
    U = np.einsum("ij,ij->i", sv, pv)
    V = np.einsum("ij,ij->i", d, np.cross(sv, f1))
    ld = np.linalg.norm(d, axis=1)
    with np.errstate(all="ignore"):
        hp = np.einsum("ij,ij->i", sv, n) / nn
        hq = np.einsum("ij,ij->i", sv + d, n) / nn
        plane = np.minimum(np.abs(hp), np.abs(hq)) * np.where(hp * hq <= 0, 1.0, -1.0)
        s = np.sign(det)
        sides = np.minimum(np.minimum(s * U / (ld * np.linalg.norm(f2, axis=1)), s * V / (ld * np.linalg.norm(f1, axis=1))),
                           s * (det - U - V) / (ld * np.linalg.norm(f2 - f1, axis=1)))
        g = np.minimum(plane, sides)
    return np.where((det != 0) & (nn > 0) & (ld > 0) & np.isfinite(g), g, -np.inf)


def margin64(rec, tris, ci, ti):
    """G of the pairs (ci[j], ti[j]): the largest of the six margins, from the float64 values of the vertices themselves"""
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)[np.asarray(ti, np.int64)]
    Q = callers(rec).astype(np.float64)[ci]
    G = np.full(len(ci), -np.inf)
    for t in six_tests(Q, T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]):
        G = np.maximum(G, seg_margin64(*t))
    return G


# ---- exact rationals, for lattice inputs ----------------------------------------------------------------------------------------------
def _fr(v):
    return [Fraction(float(x)) for x in v]


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _crossf(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dotf(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def seg_crosses_exact(p, d, a, f1, f2):
    pv = _crossf(d, f2)
    det = _dotf(f1, pv)
    sv = _sub(p, a)
    U = _dotf(sv, pv)
    qv = _crossf(sv, f1)
    V, T = _dotf(d, qv), _dotf(f2, qv)
    if det > 0:
        return U >= 0 and V >= 0 and U + V <= det and 0 <= T <= det
    if det < 0:
        return U <= 0 and V <= 0 and U + V >= det and 0 >= T >= det
    return False


def edges_exact(caller, mesh):
    """`edges` of one pair in exact arithmetic, the box stage included (0 when it fails): caller, mesh: 3 x 3 vertices"""
    q0, q1, q2 = (_fr(v) for v in np.asarray(caller, np.float64).reshape(3, 3))
    v0, v1, v2 = (_fr(v) for v in np.asarray(mesh, np.float64).reshape(3, 3))
    for k in range(3):
        if min(v0[k], v1[k], v2[k]) > max(q0[k], q1[k], q2[k]) or max(v0[k], v1[k], v2[k]) < min(q0[k], q1[k], q2[k]):
            return 0
    e1, e2, a, c = _sub(v1, v0), _sub(v2, v0), _sub(q1, q0), _sub(q2, q0)
    tests = [(q0, a, v0, e1, e2), (q1, _sub(q2, q1), v0, e1, e2), (q2, _sub(q0, q2), v0, e1, e2),
             (v0, e1, q0, a, c), (v1, _sub(e2, e1), q0, a, c), (v0, e2, q0, a, c)]
    return sum(1 << bit for bit, t in enumerate(tests) if seg_crosses_exact(*t))
