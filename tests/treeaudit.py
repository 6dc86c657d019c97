"""An exhaustive audit of a BVH as the traversal sees it: every triangle of every tree, not the rays a test happens to sample.

Four checks, all O(N) on the reference side, numpy and float64 only -- no oracle, no product code:

1. verify_bvh4 / verify_bvh2: a proof on the words read back from the device (read_bvh4 / read_bvh2).  Topology (every reachable node
   reached once, every triangle in exactly one reachable leaf, child counts, pre-order for trees this library builds); transitive
   containment (the three vertices of every triangle inside the exactly decoded f16 box of EVERY ancestor on its root path, the one
   exemption being the f16 subnormal flush of DESIGN.md section 3); and no stale or loose box (every box is what the rules of
   DESIGN.md sections 3 and 14 give, stated in the ordered-integer form of f16).  Vectorised level by level.
2. aimed_rays / judge: four rays aimed at every triangle, traced by the code under test and judged by float64 Moeller-Trumbore
   (pathref.pair) against that triangle alone, and against the triangle the code reported.
3. near_points / far_points / judge_closest, judge_radius, judge_knn, judge_counts / audit_points: the origins of those rays, and one point
   farther above every centroid, through the closest-point, radius, k-nearest and crossing-count queries, judged by float64 point-triangle
   distances (closestref) against that triangle and the reported ones alone: O(points + listed entries).

4. through_rays / aimed_surfels / judge_hits, judge_occlusion / audit_lists: the aimed rays made long (from outside the scene's box, t_max =
   +inf) through list_hits, sorted and unsorted, and the counting walk behind count_hits and contains; the aimed rays as surfels through
   occlusion (the sample rays are the product's occlusion_rays_host, the one piece of product code on the reference side: it is pinned to
   numpy bit for bit and is no part of any walk); contains, signed_distance and occlusion against their compositions.  Judged by float64 Moeller-Trumbore against the own
   triangle and the listed ones alone: O(rays + listed entries).

The megakernel's own traversal (pt_megakernel_loop.inc) cannot be reached by caller rays, so check 2 does not cover it; it stays covered by
the sampled pathref renders and by bit equality with the other kernels over the same arena, which check 1 does cover.

Test helper, not product code and not a conftest."""
import time

import numpy as np

import closest_cases as clc
import closestref
import pathref
from refit_cases import INVALID, LEAF, halves, ord16, unord16

TINY = 2.0 ** -14                    # the smallest normal f16: bounds below it are flushed to a signed zero by half_trunc
ORD_PINF, ORD_NINF = int(ord16(0x7C00)), int(ord16(0xFC00))
MISS = 0xFFFFFFFF


def decode(words):
    """(.., 3) box words -> (.., 6) float64, every f16 exactly: mn.x mn.y mn.z mx.x mx.y mx.z"""
    return halves(words).astype(np.uint16).view(np.float16).astype(np.float64)


def leaf_rule(tris, t):
    """RTNE f16 of the min / max of the three vertices (-0 below +0), one f16 step outwards, always.  -> (len(t), 6) ordered integers."""
    v = np.asarray(tris, np.float32).reshape(-1, 3, 3)[t]
    with np.errstate(over="ignore"):
        o = ord16(v.astype(np.float16).view(np.uint16))
    return np.concatenate([o.min(1) - 1, o.max(1) + 1], -1)


class _Tree:
    def __init__(self, words, stride):
        w = np.asarray(words, np.uint32)
        self.m = m = int(w[0])
        self.K = K = stride - 4
        assert len(w) >= 1 + stride * m, "the buffer is shorter than its node count says"
        rec = w[1:1 + stride * m].reshape(m, stride)
        self.kids = rec[:, 3:3 + K].astype(np.int64)
        self.meta = rec[:, 3 + K]
        self.leaf = (self.meta & LEAF) != 0
        self.tri = (self.meta & 0x7FFFFFFF).astype(np.int64)
        self.o = ord16(halves(rec[:, :3]))
        self.val = decode(rec[:, :3])
        self.ok = (self.kids != INVALID) & (self.kids < m) & ~self.leaf[:, None]      # the children the traversal fetches

    def rule(self, nodes, child_o):
        """The box of internal `nodes` from the ordered boxes `child_o` of their children: BVH4 the union from +-inf with the subnormal
        flush (collapse_up_kernel, half_trunc), BVH2 the union stepped once outwards (propagateUp)."""
        k = self.kids[nodes]
        ok = self.ok[nodes]
        ko = child_o[np.where(ok, k, 0)]
        lo = np.where(ok[..., None], ko[..., :3], 1 << 20).min(1)
        hi = np.where(ok[..., None], ko[..., 3:], -(1 << 20)).max(1)
        if self.K == 2:
            return np.concatenate([lo - 1, hi + 1], -1)
        h = unord16(np.concatenate([np.minimum(lo, ORD_PINF), np.maximum(hi, ORD_NINF)], -1))
        return ord16(np.where((h & 0x7C00) == 0, h & 0x8000, h))


class TreeReport:
    """What verify_bvh4 / verify_bvh2 found.  errors: topology, as text.  outside / exempt: (tri, node, stick-out) of every (triangle,
    ancestor) pair whose box the triangle leaves -- beyond, or within, the flush exemption.  stale: nodes whose box is not the rule's
    (stale_loose: it contains the rule's box; otherwise it is too tight somewhere).  parent, depth (-1: not reachable), leaf_of (per triangle)."""

    def perfect(self, exact=True):
        return not self.errors and len(self.outside) == 0 and (not exact or len(self.stale) == 0)

    def summary(self):
        return "%s: %d nodes (%d reachable, depth %d), %d triangles; %d topology errors, %d (triangle, ancestor) pairs outside, %d within the flush exemption (%d triangles), %d stale boxes (%d loose); %.2f s" % (
            self.kind, self.m, int((self.depth >= 0).sum()), int(self.depth.max()), self.n, len(self.errors), len(self.outside), len(self.exempt),
            len(np.unique(self.exempt["tri"])), len(self.stale), int(self.stale_loose.sum()), self.seconds)

    def leaves_box_of(self, tri):
        """The ancestors whose box triangle `tri` leaves beyond the exemption."""
        return self.outside["node"][self.outside["tri"] == tri]


PAIR = np.dtype([("tri", np.int64), ("node", np.int64), ("stick", np.float64)])


def _verify(tris, words, stride, built, kind):
    t0 = time.time()
    tr = _Tree(words, stride)
    V = np.asarray(tris, np.float32).reshape(-1, 3, 3).astype(np.float64)
    n, m, K = len(V), tr.m, tr.K
    r = TreeReport()
    r.kind, r.n, r.m, r.errors = kind, n, m, []
    err = r.errors.append

    # ---- the walk from the root, a level per step ----
    parent = np.full(m, -1, np.int64); depth = np.full(m, -1, np.int64); visits = np.zeros(m, np.int64)
    levels = []
    front = np.zeros(1, np.int64)
    depth[0] = 0; visits[0] = 1
    while len(front):
        levels.append(front)
        inner = front[~tr.leaf[front]]
        ok = tr.ok[inner]
        c = tr.kids[inner][ok]
        p = np.repeat(inner, K).reshape(-1, K)[ok]
        np.add.at(visits, c, 1)
        new = depth[c] < 0
        cu, first = np.unique(c[new], return_index=True)
        depth[cu] = len(levels); parent[cu] = p[new][first]
        front = cu
    reach = depth >= 0
    r.parent, r.depth = parent, depth
    if (visits > 1).any():
        err("%d nodes are reached more than once, first %s" % (int((visits > 1).sum()), np.flatnonzero(visits > 1)[:5].tolist()))

    # ---- topology ----
    rleaf = np.flatnonzero(reach & tr.leaf & (tr.tri < n))
    count = np.bincount(tr.tri[rleaf], minlength=n)
    if not np.all(count == 1):
        err("%d triangles sit in no reachable leaf, %d in several; first %s" % (int((count == 0).sum()), int((count > 1).sum()), np.flatnonzero(count != 1)[:5].tolist()))
    leaf_of = np.full(n, -1, np.int64)
    leaf_of[tr.tri[rleaf][::-1]] = rleaf[::-1]
    r.leaf_of = leaf_of
    rinner = np.flatnonzero(reach & ~tr.leaf)
    present = tr.kids[rinner] != INVALID
    cnt = tr.ok[rinner].sum(1)
    if not np.all(tr.ok[rinner] == present):
        err("internal nodes name children beyond the node count")
    if K == 2 and not np.all(cnt == 2):
        err("BVH2 internal nodes without exactly two children: %s" % rinner[cnt != 2][:5].tolist())
    if K == 4 and not (np.all(cnt >= 2) and np.all(cnt <= 4) and np.all(present[:, :-1] >= present[:, 1:])):
        err("BVH4 internal nodes without 2..4 children packed to the front: %s" % rinner[(cnt < 2) | (present[:, :-1] < present[:, 1:]).any(1)][:5].tolist())
    if built:
        if not reach.all():
            err("%d nodes of a built tree are not reachable" % int((~reach).sum()))
        if (tr.leaf & (tr.tri >= n)).any():
            err("a built tree has leaves beyond the triangle count")
        if not np.all(tr.meta[~tr.leaf] == 0):
            err("internal nodes with a non-zero last word")
        if K == 4:
            if not np.all(tr.kids[tr.leaf] == INVALID):
                err("leaves with child words")
            # DFS pre-order: the first child is the next node, every further child starts where its sibling's subtree ended
            size = np.ones(m, np.int64)
            for lv in levels[:0:-1]:
                np.add.at(size, parent[lv], size[lv])
            k = tr.kids[rinner]
            good = k[:, 0] == rinner + 1
            for s in range(1, 4):
                here = tr.ok[rinner][:, s]
                prev = np.where(here, k[:, s - 1], 0)
                good &= ~here | (k[:, s] == prev + size[prev])
            if not good.all():
                err("not in DFS pre-order at nodes %s" % rinner[~good][:5].tolist())
        else:
            if m != 2 * n - 1 or not np.array_equal(tr.leaf, np.arange(m) >= n - 1):
                err("BVH2 layout: internal nodes 0..N-2, leaves N-1.. expected")

    # ---- no stale or loose boxes: the rules, from the triangles upwards and from the stored children ----
    eo = tr.o.copy()
    eo[rleaf] = leaf_rule(tris, tr.tri[rleaf])
    has = tr.ok.any(1)
    for lv in levels[::-1]:
        nodes = lv[~tr.leaf[lv] & has[lv]]
        if len(nodes):
            eo[nodes] = tr.rule(nodes, eo)
    local = tr.o.copy()
    nodes = rinner[has[rinner]]
    if len(nodes):
        local[nodes] = tr.rule(nodes, tr.o)
    local[rleaf] = eo[rleaf]
    # a box is right if it is the rule over its stored children, or the rule over the triangles below it: by induction from the leaves a
    # tree without a flag equals the rule's tree word for word, and damage is flagged where it is, not at every ancestor it leaks into
    bad = reach & (tr.o != local).any(1) & (tr.o != eo).any(1)
    r.stale = np.flatnonzero(bad)
    r.stale_loose = np.all(tr.o[r.stale, :3] <= eo[r.stale, :3], 1) & np.all(tr.o[r.stale, 3:] >= eo[r.stale, 3:], 1)
    r.expected = eo

    # ---- transitive containment: every triangle climbs its root path ----
    vlo, vhi = V.min(1), V.max(1)
    act = np.flatnonzero(leaf_of >= 0)
    cur = leaf_of[act]
    found = []
    while len(act):
        b = tr.val[cur]
        lo, hi = b[:, :3], b[:, 3:]
        with np.errstate(invalid="ignore"):
            out = np.concatenate([~(lo <= vlo[act]), ~(hi >= vhi[act])], 1)
            stick = np.concatenate([lo - vlo[act], vhi[act] - hi], 1)
        rows = np.flatnonzero(out.any(1))
        if len(rows):
            st = np.where(out[rows], np.where(np.isnan(stick[rows]), np.inf, stick[rows]), 0.0)
            flushed = (b[rows] == 0) & (st < TINY)                           # a bound that is exactly +-0, exceeded by less than 2^-14
            e = np.zeros(len(rows), np.dtype(PAIR.descr + [("exempt", bool)]))
            e["tri"], e["node"], e["stick"], e["exempt"] = act[rows], cur[rows], st.max(1), np.all(~out[rows] | flushed, 1)
            found.append(e)
        cur = parent[cur]
        keep = cur >= 0
        act, cur = act[keep], cur[keep]
    f = np.concatenate(found) if found else np.zeros(0, np.dtype(PAIR.descr + [("exempt", bool)]))
    r.exempt = f[f["exempt"]][["tri", "node", "stick"]]
    r.outside = f[~f["exempt"]][["tri", "node", "stick"]]
    r.seconds = time.time() - t0
    return r


def verify_bvh4(tris, bvh4, built=True):
    """The words of read_bvh4().  built=False: a tree installed with set_bvh4, held only to what DESIGN.md section 14 promises -- nodes
    no path from the root reaches may exist, ids need not be in pre-order."""
    return _verify(tris, bvh4, 8, built, "BVH4")


def verify_bvh2(tris, bvh2, built=True):
    return _verify(tris, bvh2, 6, built, "BVH2")


def assert_tree(r, name, exact=True):
    """A perfect tree.  exact=False for an installed tree whose boxes were made by other rules (a BVH4_wide promotion before its first
    update keeps the BVH2's boxes): containment and topology only."""
    print("%s %s" % (name, r.summary()))
    assert not r.errors, "%s: %s" % (name, "; ".join(r.errors))
    assert len(r.outside) == 0, "%s: %d (triangle, ancestor) pairs outside beyond the flush exemption, first (tri, node, stick-out) %s" % (name, len(r.outside), r.outside[:5].tolist())
    if exact:
        assert len(r.stale) == 0, "%s: %d boxes are not the rule's (%d of them loose), first nodes %s" % (name, len(r.stale), int(r.stale_loose.sum()), r.stale[:5].tolist())


# ---- aimed rays -----------------------------------------------------------------------------------------------------------------------
H_REL = 1e-4
BARY = np.array([[1 / 3, 1 / 3, 1 / 3], [0.9, 0.05, 0.05], [0.05, 0.9, 0.05], [0.05, 0.05, 0.9]])


class Rays:
    """O, D (R, 3) and t_max (R,) in f32; tri (R,): the triangle ray i is aimed at (rays of a triangle are consecutive); P: the aimed point, f64."""


def aimed_rays(tris, k=4, h=H_REL):
    """k <= 4 rays per triangle: at the centroid and at the points with barycentrics (0.9, 0.05, 0.05) and its permutations.  Origin
    p + s h' n, direction -s n (n the unit geometric normal, s = +1 for even and -1 for odd triangles), t_max = 2 h',
    h' = h max(1, |p|inf); everything rounded to f32 before anybody sees it.

    h = 1e-4, chosen from the reference alone.  It has to clear pathref's margins: t and t_max - t are both h', against
    mt = max(D_T, COND_ULPS 2^-24 kappa e / |d|), which for a ray along the normal is about 1e-6 (|o| + |v0| + e) e^2 / 2A.  At unit scale
    that is below 1e-4 up to e^2 / 2A of about 30 (longest edge squared over twice the area); a sliver beyond that gets h' = 2 mt instead
    (0.5 % of the triangles of a random soup, by up to 27 times; never more than 1000 times, beyond which the triangle stays not
    auditable).  And it has to keep occluders rare: a segment of 2e-4 meets another triangle of the 120,000-triangle soup (size 0.2 in
    [-1, 1]^3, about 30 triangle crossings per unit length) in well under 1 % of the rays.
    Measured -- rays not auditable / answered by an occluder, a duplicate or a triangle at a margin / triangles without any auditable
    ray; float64 reference over the host twins and the oracle's traversal (tests/test_tree_audit.py), closest hit:
      soups 1 .. 2,500, 30,000 and 120,000 (size 0.2)  0 % / 0 - 0.03 % / 0 %     (120,000: 0 of 1,500 sampled rays answered by an occluder, by brute force)
      dragon-class 1,500 - 3,000, sponza-class 12,000  0 % / 0 % / 0 %            (0.15 % occluders after eight waves of amplitude 0.32)
      room, cornell, f16 grid                          0 % / 0 % / 0 %            (exactly axis-parallel rays)
      soup of size 2 in [980, 1020]^3                  0.49 % / 0.11 % / 0 %      (|o| / e conditions a pair: at size 0.2 a third of the corner rays are not auditable)
      soup x 27,000                                    0 % / 0 % / 0 %
      a cluster of 1 % collapsed to a point            1 % / 0 % / 1 %            (zero area: unhittable by the specification)
      C2 (871,414) and C4 (262,144), reference only    0 % not auditable, 0 % without an auditable ray
    The DEGENERATE families are outside what any h can audit and are classed, not capped (test_tree_audit.check_family): tiny 100 % not
    auditable (|e1 x e2| of 1e-11 against the 1e-7 determinant threshold); identical 99.7 % answered by a duplicate; coplanar 94 %,
    signed_zero 53 %, two_clusters 80 % answered by a coplanar or nearer triangle; mixed_zero 6.8 % without area, 25 % answered by another."""
    T = np.asarray(tris, np.float32).reshape(-1, 3, 3).astype(np.float64)
    n = len(T)
    c = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    ln = np.sqrt((c * c).sum(1))
    with np.errstate(all="ignore"):
        nrm = np.where((ln > 0)[:, None] & np.isfinite(ln)[:, None], c / ln[:, None], np.array([0.0, 0.0, 1.0]))
    P = np.einsum("kj,njc->nkc", BARY[:k], T)
    s = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    hh = h * np.maximum(1.0, np.abs(P).max(-1))
    # a sliver's own margin of t (pathref's mt for a unit direction along the normal, |det| = |e1 x e2|) can exceed that: such a ray starts
    # twice its margin away instead, as long as that stays a small step (a tenth of the scale); beyond it the triangle is left not auditable
    E = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]], 1)
    em = np.sqrt((E ** 2).sum(-1).max(1))
    with np.errstate(all="ignore"):
        mt = pathref.COND_ULPS * pathref.U32 * (em * em / ln)[:, None] * (np.sqrt((P ** 2).sum(-1)) + hh + np.sqrt((T[:, 0] ** 2).sum(1))[:, None] + em[:, None])
    hh = np.where(np.isfinite(mt) & (2 * mt > hh) & (2 * mt <= 1000 * hh), 2 * mt, hh)
    r = Rays()
    r.O = (P + (s[:, None] * hh)[..., None] * nrm[:, None, :]).astype(np.float32).reshape(-1, 3)
    r.D = np.repeat((-s[:, None] * nrm).astype(np.float32), k, 0)
    r.t_max = (2 * hh).astype(np.float32).reshape(-1)
    r.tri = np.repeat(np.arange(n), k)
    r.P = P.reshape(-1, 3)
    r.k, r.n, r.own = k, n, None
    return r


def margins(tris, O, D, prim, t_max):
    """pathref._candidates for the pair (ray i, triangle prim[i]) alone, elementwise: -> dict(acc, loose, tight, t, u, v, mt, mb, det)."""
    det, u, v, t = pathref.pair(tris, O, D, prim)
    T = np.asarray(tris, np.float32).reshape(-1, 3, 3)[np.asarray(prim, np.int64)].astype(np.float64)
    o = np.asarray(O, np.float32).astype(np.float64); d = np.asarray(D, np.float32).astype(np.float64)
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    em = np.sqrt(np.maximum((e1 ** 2).sum(1), (e2 ** 2).sum(1)))
    v0n = np.sqrt((T[:, 0] ** 2).sum(1)); dn = np.sqrt((d * d).sum(1)); on = np.sqrt((o * o).sum(1))
    b0 = np.minimum(np.asarray(t_max, np.float32).astype(np.float64), pathref.INF_T)
    eps = pathref.EPS_T
    with np.errstate(all="ignore"):
        adet = np.abs(det)
        kap = dn * em * (on + v0n + em) / adet
        mb = np.maximum(pathref.D_B, pathref.COND_ULPS * pathref.U32 * kap)
        mt = np.maximum(pathref.D_T, pathref.COND_ULPS * pathref.U32 * kap * em / dn)
        bary = np.minimum(np.minimum(u, 1 - u), np.minimum(v, 1 - u - v))
        acc = (adet >= eps) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > eps) & (t < b0)
        loose = (adet >= eps - pathref.D_DET) & (bary > -mb) & (t > eps - mt) & (t < b0 + mt)
        tight = (adet >= eps + pathref.D_DET) & (bary >= mb) & (t >= eps + mt) & (t <= b0 - mt)
    return dict(acc=acc, loose=loose | acc, tight=tight, t=t, u=u, v=v, mt=mt, mb=mb, det=det)


class Judgement:
    """Per ray: auditable (the reference accepts its own triangle with every margin to spare), own (the code reported it), occluder (it
    reported another triangle the reference accepts for certain no farther), fragile (it reported a triangle at a margin of the
    reference: a knife edge by pathref's rules, not comparable), lost.  lost_tris: the triangles of the lost rays."""

    def summary(self):
        return "%d triangles (%d audited), %d rays: not auditable %.3f %%, answered by an occluder or duplicate %.3f %% (%d rays), at a margin %.3f %%, ill-conditioned values %.3f %%; triangles without an auditable ray %.3f %%; lost rays %d (triangles %d); reference %.2f s" % (
            self.n, self.n - int(round(self.share_blind_tris * self.n)), self.R, 100 * self.share_not_auditable, 100 * self.share_occluder, int((self.auditable & (self.occluder | self.fragile)).sum()), 100 * self.fragile.mean() if self.R else 0.0,
            100 * self.poor.mean() if self.R else 0.0, 100 * self.share_blind_tris, len(self.lost), len(self.lost_tris), self.seconds)


def judge(tris, rays, got, any_hit=False):
    """got = (t, prim, u, v) as trace_rays returns them.  O(rays): float64 Moeller-Trumbore of each ray against its own triangle and
    against the reported one, nothing else."""
    t0 = time.time()
    t, prim, u, v = [np.asarray(a) for a in got]
    n, R = rays.n, len(rays.tri)
    if rays.own is None:                                                         # the same for every kernel and hit type: once per ray set
        rays.own = margins(tris, rays.O, rays.D, rays.tri, rays.t_max)
    own = rays.own
    j = Judgement()
    j.n, j.R, j.any_hit, j.tri = n, R, any_hit, rays.tri
    aud = j.auditable = own["tight"]
    got_hit = prim != MISS
    inrange = got_hit & (prim < n)
    is_own = got_hit & (prim.astype(np.int64) == rays.tri)
    oth = np.flatnonzero(inrange & ~is_own)
    j.occluder = np.zeros(R, bool); j.fragile = np.zeros(R, bool); j.poor = np.zeros(R, bool); j.values_off = np.zeros(0, np.int64)
    phantom = got_hit & ~inrange
    if any_hit:
        # it must hit, and the reference must accept the reported triangle below t_max
        h = np.flatnonzero(inrange)
        okh, th = pathref.loosely_accepts(tris, rays.O[h], rays.D[h], prim[h], rays.t_max[h])
        good = np.zeros(R, bool); good[h] = okh
        j.occluder[oth] = good[oth]
        j.lost = np.flatnonzero(aud & ~good)
        phantom |= got_hit & ~good & ~aud
    else:
        m = margins(tris, rays.O[oth], rays.D[oth], prim[oth], rays.t_max[oth])
        ti, mti = own["t"][oth], own["mt"][oth]
        with np.errstate(invalid="ignore"):
            sure = m["tight"] & (m["t"] <= ti + pathref.D_T)
            edge = ~sure & m["loose"] & (~aud[oth] | (m["t"] < (ti + mti) + m["mt"]))
        j.occluder[oth] = sure
        j.fragile[oth] = edge
        phantom[oth[~sure & ~edge & ~aud[oth]]] = True                         # a ray that is not auditable is still explained
        j.lost = np.flatnonzero(aud & ~is_own & ~j.occluder & ~j.fragile)
        # values, where plain f32 can deliver them: the reference's own f32 evaluation of the pair within TOL / 4 (QueryRef.poor's rule)
        s = np.flatnonzero(aud & is_own)
        _, u32, v32, t32 = pathref.pair(tris, rays.O[s], rays.D[s], rays.tri[s], np.float32)
        q = pathref.TOL / 4
        tr, ur, vr = own["t"][s], own["u"][s], own["v"][s]
        with np.errstate(invalid="ignore"):
            j.poor[s] = ~((np.abs(u32 - ur) <= q) & (np.abs(v32 - vr) <= q) & (np.abs(t32 - tr) <= q * np.maximum(tr, 1)))
            off = ~j.poor[s] & ~((np.abs(t[s] - tr) <= pathref.TOL * np.maximum(tr, 1)) & (np.abs(u[s] - ur) <= pathref.TOL) & (np.abs(v[s] - vr) <= pathref.TOL))
        j.values_off = s[off]
    j.phantom = np.flatnonzero(phantom)
    j.lost_tris = np.unique(rays.tri[j.lost])
    j.share_not_auditable = float((~aud).mean()) if R else 0.0
    j.share_occluder = float((aud & (j.occluder | j.fragile)).mean()) if R else 0.0
    j.share_blind_tris = float((np.bincount(rays.tri[aud], minlength=n) == 0).mean()) if n else 0.0
    j.seconds = time.time() - t0
    return j


def assert_judged(j, name, tree=None, capped=True):
    """No lost triangle, no hit the reference cannot explain, values within pathref.TOL; and (capped) the rays this audit cannot use --
    not auditable, or answered by an occluder -- at most pathref.FRAGILE_CAP of the case, as are triangles without any auditable ray."""
    lost, flushed = j.lost_tris, np.zeros(0, np.int64)
    if tree is not None:
        # a loss the containment proof attributes to the subnormal flush is the reference's behaviour: counted within the cap, not a failure
        mine = np.isin(lost, tree.exempt["tri"]) & ~np.isin(lost, tree.outside["tri"])
        lost, flushed = lost[~mine], lost[mine]
    print("%s%s %s%s" % (name, " any hit" if j.any_hit else "", j.summary(), "; %d of the lost triangles stick out of a flushed bound" % len(flushed) if len(flushed) else ""))
    if len(lost):
        why = ""
        if tree is not None:
            why = "; boxes they leave (tri -> nodes): %s" % {int(t): tree.leaves_box_of(t).tolist() for t in lost[:10]}
        raise AssertionError("%s: %d lost triangles, first %s%s" % (name, len(lost), lost[:20].tolist(), why))
    assert len(j.phantom) == 0, "%s: %d rays report a triangle the reference cannot accept, first rays %s" % (name, len(j.phantom), j.phantom[:10].tolist())
    assert len(j.values_off) == 0, "%s: t, u or v beyond pathref.TOL on %d rays, first %s" % (name, len(j.values_off), j.values_off[:10].tolist())
    if capped:
        cap = pathref.FRAGILE_CAP
        unused = j.share_not_auditable + j.share_occluder + float(np.isin(j.tri[j.lost], flushed).sum()) / max(j.R, 1)
        assert unused <= cap, "%s: %.2f %% of the rays are not auditable, answered by an occluder or lost to the flush (cap 2 %%): change the scene or h" % (name, 100 * unused)
        assert j.share_blind_tris <= cap, "%s: %.2f %% of the triangles have no auditable ray (cap 2 %%)" % (name, 100 * j.share_blind_tris)


def segment_meets_box(rays, idx, lo, hi, bounded=True, rel=1e-6):
    """Does the segment of ray idx[i] (origin to t_max; the whole ray if not `bounded`) meet the box?  float64 slabs -> (certainly yes,
    certainly no); a segment within `rel` of touching is neither.  For the detection tests: a triangle is lost exactly when its ray misses
    a box on its path.  The kernels prune a box entered beyond t_max; the oracle's probe has no t_max, so
    HostContext, which cuts the answer off afterwards, walks the whole ray (`prunes_at_t_max`)."""
    o = rays.O[idx].astype(np.float64); d = rays.D[idx].astype(np.float64); tm = rays.t_max[idx].astype(np.float64)
    with np.errstate(all="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
        par = d == 0
        near = np.where(par, np.where((o >= lo) & (o <= hi), -np.inf, np.inf), np.minimum(t1, t2)).max(1)
        far = np.where(par, np.where((o >= lo) & (o <= hi), np.inf, -np.inf), np.maximum(t1, t2)).min(1)
    a, b = np.maximum(near, 0.0), np.minimum(far, tm) if bounded else far
    slack = rel * np.maximum(1.0, np.abs(o).max(1))
    return a <= b - slack, a > b + slack


# ---- a context's tree through both checks ---------------------------------------------------------------------------------------------
KERNELS = [False, True]              # simple=False: the persistent ray-query kernel; True: one ray per lane


def audit_context(ctx, tris, name, built=True, exact=True, bvh2=True, capped=True, kernels=KERNELS, rays=None):
    """The three steps for the tree `ctx` holds over `tris` (anything with read_bvh4 / read_bvh2 / trace_rays: a device context, or the
    host twins with the oracle's traversal standing in): the words through verify_*, the aimed rays through every kernel, closest and
    any hit, through judge.  -> (BVH4 report, {(simple, any_hit): judgement})."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    r4 = verify_bvh4(tris, ctx.read_bvh4(), built)
    assert_tree(r4, name, exact)
    if bvh2:
        assert_tree(verify_bvh2(tris, ctx.read_bvh2(), built), name, exact)
    rays = aimed_rays(tris) if rays is None else rays
    out = {}
    for simple in kernels:
        for any_hit in (False, True):
            got = ctx.trace_rays(rays.O, rays.D, t_max=rays.t_max, any_hit=any_hit, simple=simple)
            out[simple, any_hit] = j = judge(tris, rays, got, any_hit)
            assert_judged(j, "%s simple %d" % (name, simple), r4, capped)
    return r4, out


class HostContext:
    """The calls of a device context that the audit uses, answered by the host twins of the build and the refit and by the oracle's
    traversal (one orc.trace_ray per ray; t_max applied as DESIGN.md section 13 defines it: a hit iff the unbounded closest hit lies below)."""

    prunes_at_t_max = False

    def __init__(self, rt, orc):
        self.rt, self.orc, self.b4, self.b2 = rt, orc, None, None

    def set_triangles(self, tris):
        self.tris = np.array(tris, np.float32).reshape(-1)
        self.n = self.tris.size // 9
        self.b4 = self.b2 = None

    def build_bvh(self, accel=0):
        self.b2 = self.rt.build_bvh2_ploc(self.tris) if accel == 2 else self.orc.build_lbvh2(self.tris)
        self.b4 = self.rt.collapse_bvh2_to_bvh4_accel(self.b2, self.n, accel)[0]

    def set_bvh4(self, bvh4):
        self.b4, self.b2 = np.array(bvh4, np.uint32), None

    def set_bvh2(self, bvh2):
        self.b2 = np.array(bvh2, np.uint32)
        self.b4 = self.rt.collapse_lbvh2_to_bvh4(self.b2, self.n)[0]

    def update_triangles(self, tris):
        self.tris = np.array(tris, np.float32).reshape(-1)
        self.b4 = self.rt.refit_bvh4(self.tris, self.b4)
        if self.b2 is not None:
            self.b2 = self.rt.refit_bvh2(self.tris, self.b2)

    def read_bvh4(self):
        return self.b4

    def read_bvh2(self):
        return self.b2

    def trace_rays(self, O, D, t_max=None, any_hit=False, simple=False):
        R = len(O)
        t = np.full(R, np.inf, np.float32); prim = np.full(R, MISS, np.uint32)
        tm = np.full(R, np.inf, np.float32) if t_max is None else np.asarray(t_max, np.float32)
        for i in range(R):
            h, tt, _, tri = self.orc.trace_ray(self.tris, self.b4, O[i], D[i], anyhit=any_hit)
            if h and any_hit and not tt < tm[i]:
                h, tt, _, tri = self.orc.trace_ray(self.tris, self.b4, O[i], D[i], anyhit=False)
            if h and tt < tm[i]:
                t[i], prim[i] = tt, tri
        hit = np.flatnonzero(prim != MISS)
        u = np.zeros(R, np.float32); v = np.zeros(R, np.float32)
        if len(hit):                                                            # the oracle's probe returns no barycentrics: the f32 evaluation of the winning pair
            _, uu, vv, _ = pathref.pair(self.tris, O[hit], D[hit], prim[hit], np.float32)
            u[hit], v[hit] = uu, vv
        return t, prim, u, v

    # ---- the point and crossing-count queries: the host twins, their counters kept for stats() as a device context keeps them ----
    def stats(self):
        return self._stats

    def _twin(self, fn, *a, **kw):
        res = fn(self.tris, self.b4, *a, stats=True, **{k: v for k, v in kw.items() if k != "stats"})
        self._stats = res[-1]
        return res[:-1]

    def closest_points(self, points, r_max=None, **kw):
        return self._twin(self.rt.closest_points_bvh4, points, r_max, **kw)

    def radius_search(self, points, r_max=None, **kw):
        return self._twin(self.rt.radius_search_bvh4, points, r_max, **kw)

    def radius_count(self, points, r_max=None, **kw):
        return np.diff(self._twin(self.rt.radius_search_bvh4, points, r_max, capacity=0, **kw)[0].astype(np.int64)).astype(np.uint32)

    def nearest_k(self, points, k, r_max=None, **kw):
        return self._twin(self.rt.nearest_k_bvh4, points, k, r_max, **kw)

    def count_hits(self, origins, directions=None, t_max=None, **kw):
        return self._twin(self.rt.count_hits_bvh4, origins, directions, t_max, **kw)[0]

    def list_hits(self, origins, directions=None, t_max=None, **kw):
        return self._twin(self.rt.list_hits_bvh4, origins, directions, t_max, **kw)

    def contains(self, points, samples=3, **kw):
        return self._twin(self.rt.contains_bvh4, points, samples, **kw)


# ---- aimed points: the point and crossing-count queries ---------------------------------------------------------------------------------
H2_REL = 16 * 2.0 ** -12             # the far pass: sixteen times the slack s = 2^-12 of bound2
K_NEAR, K_FAR = 8, 64                # nearest_k's k in the two passes


class Points:
    """P (R, 3) and r_max (R,) in f32; tri (R,): the triangle point i is aimed at; what: "near" or "far".  The float64 side, filled in by
    the first judge: tol, d_own, auditable, and a memo of every (point, triangle) distance a judge has asked for."""

    def __init__(self, tris, P, r_max, tri, what):
        self.tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
        self.P, self.r_max, self.tri, self.what = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(r_max, np.float32), np.asarray(tri, np.int64), what
        self.n, self.R = self.tris.size // 9, len(self.tri)
        self.tol = clc.tolerance(self.P, self.tris) if self.R else 0.0
        self._keys, self._d = np.zeros(0, np.int64), np.zeros(0)
        self.d_own = self.distance(np.arange(self.R), self.tri)
        r = self.r_max.astype(np.float64)
        self.auditable = (self.d_own >= 4 * self.tol) & (self.d_own <= r - 4 * self.tol)

    def records(self):
        return np.concatenate([self.P, self.r_max[:, None]], 1)

    def distance(self, idx, prim):
        """closestref.distance_to(P[idx], triangle prim), each pair evaluated once however many kernels report it."""
        keys = (np.asarray(idx, np.int64) << 32) | np.asarray(prim, np.int64)
        pos = np.minimum(np.searchsorted(self._keys, keys), max(len(self._keys) - 1, 0))
        known = self._keys[pos] == keys if len(self._keys) else np.zeros(len(keys), bool)
        out = np.empty(len(keys))
        out[known] = self._d[pos[known]]
        new, inv = np.unique(keys[~known], return_inverse=True)
        if len(new):
            d = closestref.distance_to(self.P[new >> 32], self.tris, new & 0xFFFFFFFF)
            out[~known] = d[inv]
            k = np.concatenate([self._keys, new]); order = np.argsort(k, kind="stable")
            self._keys, self._d = k[order], np.concatenate([self._d, d])[order]
        return out

    def uv_distance(self, idx, prim, u, v):
        """float64 distance from P[idx] to the point (u, v) of triangle prim."""
        return np.linalg.norm(self.P[idx].astype(np.float64) - clc.closest_point_of(self.tris, prim, u, v), axis=1)


def near_points(rays, tris):
    """The near pass: the origins of aimed_rays -- P + s h' n at the four barycentric positions, h' = H_REL max(1, |P|inf) with the sliver
    rule as it is -- with r_max = 2 h', the ray's t_max."""
    return Points(tris, rays.O, rays.t_max, rays.tri, "near")


def far_points(tris):
    """The far pass: one point per triangle, H2 = 16 * 2^-12 * max(1, |c|inf) above (even triangles) or below (odd) the centroid c, with
    r_max = 2 H2.  bound2 carries a slack of s = 2^-12, more than the near pass's r_max of about 2e-4: there every box close to the point is
    entered and pruning at the leaves' level never decides anything.  Sixteen times s makes it decide."""
    T = np.asarray(tris, np.float32).reshape(-1, 3, 3).astype(np.float64)
    n = len(T)
    c = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    ln = np.sqrt((c * c).sum(1))
    with np.errstate(all="ignore"):
        nrm = np.where((ln > 0)[:, None] & np.isfinite(ln)[:, None], c / ln[:, None], np.array([0.0, 0.0, 1.0]))
    cen = T.mean(1)
    s = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    h2 = H2_REL * np.maximum(1.0, np.abs(cen).max(-1))
    return Points(tris, cen + (s * h2)[:, None] * nrm, 2 * h2, np.arange(n), "far")


class PointJudgement:
    """Per point and query.  lost: points whose own triangle the query must have reported and did not; phantom: points with an entry the
    reference cannot accept (a triangle beyond the count, a dist or (u, v) point more than tol from the float64 distance of the reported
    triangle, a triangle beyond r_max + tol), malformed: points whose list or row breaks the form (a triangle twice, a row out of order or
    badly padded, a count that is not the list's length).  excused: auditable points that say nothing about their own triangle --
    answered by a nearer triangle (closest), a full row of certain neighbours (k-nearest); never used by the radius and count judges."""

    def summary(self):
        return "%s pass, %d triangles, %d points: not auditable %.3f %%, %s %.3f %% (%d points), lost %d (triangles %d), phantom %d, malformed %d, %d entries; reference %.2f s" % (
            self.what, self.n, self.R, 100 * self.share_not_auditable, self.excuse, 100 * self.share_excused, int(self.excused.sum()),
            len(self.lost), len(self.lost_tris), len(self.phantom), len(self.malformed), self.entries, self.seconds)

    def counts(self):
        """the figures two runs over the same bits must share"""
        return (self.R, int((~self.auditable).sum()), int(self.excused.sum()), len(self.lost), len(self.lost_tris), len(self.phantom), len(self.malformed), self.entries,
                len(getattr(self, "values_off", ())))


def _point_judgement(pts, query, excuse, t0, lost, phantom, malformed, excused, entries):
    j = PointJudgement()
    j.query, j.what, j.excuse, j.n, j.R, j.tri, j.auditable = query, pts.what, excuse, pts.n, pts.R, pts.tri, pts.auditable
    j.lost, j.phantom, j.malformed = np.flatnonzero(lost), np.flatnonzero(phantom), np.flatnonzero(malformed)
    j.excused = excused & pts.auditable
    j.lost_tris = np.unique(pts.tri[j.lost])
    j.share_not_auditable = float((~pts.auditable).mean()) if pts.R else 0.0
    j.share_excused = float(j.excused.mean()) if pts.R else 0.0
    j.entries = int(entries)
    j.seconds = time.time() - t0
    return j


def _entries_off(pts, idx, dist, prim, u, v):
    """The value rules of a reported entry (point idx[i], triangle prim[i] < n): -> (float64 distance of prim, bool: the entry is a phantom).
    |dist - d_f64| <= tol, the (u, v) point within tol of that distance (closest_cases.deviations' rule), and d_f64 <= r_max + tol."""
    d = pts.distance(idx, prim)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(dist.astype(np.float64) - d) <= pts.tol) & (np.abs(pts.uv_distance(idx, prim, u, v) - d) <= pts.tol) & (d <= pts.r_max[idx].astype(np.float64) + pts.tol)
    return d, ~ok


def judge_closest(tris, pts, got):
    """got = (dist, prim, u, v) of closest_points over pts.records().  Lost: an auditable point reports nothing, or a triangle whose float64
    distance exceeds d_own + tol.  Answered by another triangle (excused, capped): prim != own and d_f64(prim) < d_own - tol."""
    t0 = time.time()
    dist, prim, u, v = [np.asarray(a) for a in got]
    found = prim != MISS
    inr = found & (prim < pts.n)
    idx = np.flatnonzero(inr)
    d, off = _entries_off(pts, idx, dist[idx], prim[idx], u[idx], v[idx])
    phantom = found & ~inr
    phantom[idx[off]] = True
    drep = np.full(pts.R, np.inf); drep[idx] = d
    lost = pts.auditable & (drep > pts.d_own + pts.tol)
    other = inr & (prim.astype(np.int64) != pts.tri) & (drep < pts.d_own - pts.tol)
    return _point_judgement(pts, "closest_points", "answered by another triangle", t0, lost, phantom, np.zeros(pts.R, bool), other, len(idx))


def judge_radius(tris, pts, offsets, entries, counts=None):
    """offsets and entries = (dist, prim, u, v) of radius_search, counts of radius_count.  No point is excused: a nearer neighbour does not
    excuse a missing triangle.  Lost: the own triangle of an auditable point is not in its list."""
    t0 = time.time()
    off = np.asarray(offsets).astype(np.int64)
    dist, prim, u, v = [np.asarray(a) for a in entries]
    assert len(off) == pts.R + 1 and off[0] == 0 and off[-1] == len(prim) and np.all(np.diff(off) >= 0), "offsets are no offsets into the entries"
    owner = np.repeat(np.arange(pts.R), np.diff(off))
    phantom = np.zeros(pts.R, bool); malformed = np.zeros(pts.R, bool)
    inr = prim < pts.n
    phantom[owner[~inr]] = True
    d, bad = _entries_off(pts, owner[inr], dist[inr], prim[inr], u[inr], v[inr])
    phantom[owner[inr][bad]] = True
    keys = np.sort((owner << 32) | prim.astype(np.int64))
    malformed[keys[1:][keys[1:] == keys[:-1]] >> 32] = True                    # a triangle twice in one list
    if counts is not None:
        malformed |= np.asarray(counts).astype(np.int64) != np.diff(off)
    lost = pts.auditable & ~np.isin((np.arange(pts.R) << 32) | pts.tri, keys)
    return _point_judgement(pts, "radius_search", "excused", t0, lost, phantom, malformed, np.zeros(pts.R, bool), len(prim))


def judge_knn(tris, pts, rows, k):
    """rows = (dist, prim, u, v), each (R, k), of nearest_k.  Form: the listed entries first, in ascending order of
    dist, distinct triangles, then padding of dist = +inf, prim = 0xFFFFFFFF, u = v = 0.  Lost: own is absent from the row of an auditable
    point -- unless all k entries have d_f64 <= d_own + tol, a full row of certain neighbours (excused, capped)."""
    t0 = time.time()
    dist, prim, u, v = [np.ascontiguousarray(a).reshape(pts.R, k) for a in rows]
    listed = prim != MISS
    pad_ok = listed | ((dist.view(np.uint32) == 0x7F800000) & (u.view(np.uint32) == 0) & (v.view(np.uint32) == 0))
    with np.errstate(invalid="ignore"):
        malformed = ~pad_ok.all(1) | (listed[:, :-1] < listed[:, 1:]).any(1) | (listed[:, 1:] & ~(dist[:, :-1] <= dist[:, 1:])).any(1)
    p64 = np.where(listed, prim.astype(np.int64), (1 << 40) + np.arange(k)[None, :])
    srt = np.sort(p64, 1)
    malformed |= (srt[:, 1:] == srt[:, :-1]).any(1)
    inr = listed & (prim < pts.n)
    pi, col = np.nonzero(inr)
    d, bad = _entries_off(pts, pi, dist[pi, col], prim[pi, col], u[pi, col], v[pi, col])
    phantom = (listed & ~inr).any(1)
    phantom[pi[bad]] = True
    drow = np.full((pts.R, k), np.inf); drow[pi, col] = d
    has_own = (p64 == pts.tri[:, None]).any(1)
    crowded = ~has_own & (drow <= (pts.d_own + pts.tol)[:, None]).all(1)
    lost = pts.auditable & ~has_own & ~crowded
    return _point_judgement(pts, "nearest_k %d" % k, "a full row of certain neighbours", t0, lost, phantom, malformed, crowded, len(pi))


def judge_counts(rays, counts, tris=None):
    """counts of count_hits over the aimed rays (t_max = 2 h').  Lost: a count of 0 on a ray whose own triangle margins() accepts with every
    margin to spare (rays.own, computed once per ray set)."""
    t0 = time.time()
    if rays.own is None:
        rays.own = margins(tris, rays.O, rays.D, rays.tri, rays.t_max)
    counts = np.asarray(counts)
    j = PointJudgement()
    j.query, j.what, j.excuse, j.n, j.R, j.tri, j.auditable = "count_hits", "near", "excused", rays.n, len(rays.tri), rays.tri, rays.own["tight"]
    j.lost = np.flatnonzero(j.auditable & (counts == 0))
    j.phantom = j.malformed = np.zeros(0, np.int64)
    j.excused = np.zeros(j.R, bool)
    j.lost_tris = np.unique(rays.tri[j.lost])
    j.share_not_auditable = float((~j.auditable).mean()) if j.R else 0.0
    j.share_excused, j.entries, j.seconds = 0.0, int(counts.sum()), time.time() - t0
    return j


def assert_point_judged(j, name, tree=None, capped=True):
    """No lost triangle, no phantom, no malformed list; and (capped) the points this audit cannot use -- not auditable, answered by another
    triangle, a full row of certain neighbours -- each at most pathref.FRAGILE_CAP of the case.  `tree`: a TreeReport, or a function that
    makes one, asked only when a triangle is lost."""
    print("%s %s %s" % (name, j.query, j.summary()))
    if len(j.lost_tris):
        if callable(tree):
            tree = tree()
        why = "" if tree is None else "; boxes they leave (tri -> nodes): %s" % {int(t): tree.leaves_box_of(t).tolist() for t in j.lost_tris[:10]}
        raise AssertionError("%s %s, %s pass: %d lost triangles, first %s%s" % (name, j.query, j.what, len(j.lost_tris), j.lost_tris[:20].tolist(), why))
    assert len(j.phantom) == 0, "%s %s, %s pass: %d points report an entry the reference cannot accept, first points %s" % (name, j.query, j.what, len(j.phantom), j.phantom[:10].tolist())
    assert len(j.malformed) == 0, "%s %s, %s pass: %d points with a malformed list, row or count, first points %s" % (name, j.query, j.what, len(j.malformed), j.malformed[:10].tolist())
    off = getattr(j, "values_off", ())                                          # judge_hits only: t, u or v of a certain entry beyond the pair's own margin
    assert len(off) == 0, "%s %s: t, u or v beyond the pair's margin on %d rays (worst %.3f of it), first %s" % (name, j.query, len(off), j.worst, off[:10].tolist())
    if capped:
        blind = getattr(j, "share_blind_tris", 0.0)                             # judge_occlusion only
        assert blind <= pathref.FRAGILE_CAP, "%s %s: %.2f %% of the triangles have no auditable surfel (cap 2 %%)" % (name, j.query, 100 * blind)
        cap = pathref.FRAGILE_CAP
        assert j.share_not_auditable <= cap, "%s %s, %s pass: %.2f %% of the points are not auditable (cap 2 %%): change the scene or the distance" % (name, j.query, j.what, 100 * j.share_not_auditable)
        assert j.share_excused <= cap, "%s %s, %s pass: %.2f %% of the points are %s (cap 2 %%): change the scene or the distance" % (name, j.query, j.what, 100 * j.share_excused, j.excuse)


def bound2_f64(p, lo, hi, s=2.0 ** -12):
    """bound2 of DESIGN.md section 15 restated in float64, slack included: per axis g = max(mn - (p + s), (p - s) - mx, 0), the sum of the squares."""
    p = np.asarray(p, np.float64)
    g = np.maximum(np.maximum(lo - (p + s), (p - s) - hi), 0.0)
    return (g * g).sum(-1)


def point_queries(ctx, pts, rays, simple, k, stats=False, closest=True):
    """The five calls over one pass, as their judges take them: -> dict(closest, count, search, knn[, hits]; drops: stack_drops per call with stats)."""
    rec = pts.records()
    out, drops = {}, []

    def run(key, call, *a, **kw):
        out[key] = call(*a, simple=simple, stats=stats, **kw)
        if stats:
            drops.append(int(ctx.stats()["stack_drops"]))
    if closest:
        run("closest", ctx.closest_points, rec)
    run("count", ctx.radius_count, rec)
    run("search", ctx.radius_search, rec)
    run("knn", ctx.nearest_k, rec, k)
    if rays is not None:
        run("hits", ctx.count_hits, rays.O, rays.D, t_max=rays.t_max)
    out["drops"] = drops
    return out


def judge_points(tris, pts, rays, res, k):
    """-> {query: judgement} for one point_queries result."""
    out = dict(radius=judge_radius(tris, pts, res["search"][0], res["search"][1:], res["count"]), knn=judge_knn(tris, pts, res["knn"], k))
    if "closest" in res:
        out["closest"] = judge_closest(tris, pts, res["closest"])
    if "hits" in res:
        out["hits"] = judge_counts(rays, res["hits"], tris)
    return out


def audit_points(ctx, tris, name, rays=None, kernels=KERNELS, capped=True, tree=None, far_closest=True, passes=None):
    """Every triangle through the point and crossing-count queries of `ctx` (a device context or HostContext): the near pass (the origins of
    the aimed rays, r_max = 2 h', k = 8; the same records as rays through count_hits) and the far pass (far_points, k = 64), each through
    closest_points, radius_count + radius_search and nearest_k of every kernel in `kernels`, each result through its judge.  The counting
    variant of every query runs once per pass and must drop nothing at the 64-entry cap: everything the judges hold is what a walk without
    drops owes.  -> {(pass, simple): {query: judgement}}.

    Measured on the CPU over the host twins, all points, built and refitted after `wave` and `deform`, accel 0, 1 and 2 (tests/test_point_audit.py
    prints them) -- points not auditable / answered by another triangle (closest) / a full row of certain neighbours (k-nearest):
      (no point of any scene below was not auditable, no k-nearest row was full of certain neighbours: 0 % / . / 0 % throughout; the figures
      are the closest-point shares, built / after wave / after deform, the largest of the three accel levels)
                                        near pass                      far pass
      soups 1, 2, 3, 4, 5, 64, 65       0 / 0 / 0 %                    0 / 0 / 0 %
      soup 777                          0 / 0.03 / 0.03 %              0.39 / 0.64 / 0.77 %
      soup 30,000 (size 0.2)            0.41 / 0.46 / 0.32 %           17.8 / 19.3 / 10.2 %      no far closest; deform is of the same soup at size 0.1
                                                                                                 (at size 0.2 it gives 1.01 % in the near pass)
      soup 30,000, size 0.02            0.002 / 0.002 / 0.015 %        0.58 / 0.64 / 1.13 %      no far closest after deform
      soup 120,000, size 0.02           0.016 / 0.020 / 0.061 %        2.41 / 2.58 / 4.47 %      no far closest
      dragon-class 20,000               0 / 0 / 0.04 %                 0.17 / 0.35 / 3.62 %      no far closest after deform
      sponza-class 12,000               0 / 0 / (2.98 %)               10.6 / 10.7 / (16.6 %)    no far closest; deform is outside the capped audit:
                                                                                                 test_point_audit.test_deformed_sponza_slivers
      f16 grid                          0 / 0 / 0 %                    0 / 0 / 0.52 %
    A scene or a pass above 1 % is changed, never the cap, which is asserted wherever closest_points is judged.  far_closest=False: the far
    pass of this case has another triangle within 16 * 2^-12 of more than 1 % of its centroids -- the scene's density, which no distance of
    this pass can avoid -- so closest_points is not part of its far pass (not called, not judged); radius_search and nearest_k, which excuse
    nothing there, and everything of the near pass still are.  The far pass of closest_points is carried by the cases under 1 %: the small soups,
    soup 30,000 at size 0.02 (built, wave), the dragon-class scene (built, wave), the f16 grid.
    passes: (near, far) Points made before, whose float64 side is then shared."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    rays = aimed_rays(tris) if rays is None else rays
    if tree is None:
        tree = lambda: verify_bvh4(tris, ctx.read_bvh4(), built=False)
    out = {}
    near, far = passes if passes is not None else (near_points(rays, tris), far_points(tris))
    for pts, k, rr in ((near, K_NEAR, rays), (far, K_FAR, None)):
        closest = far_closest or pts.what == "near"
        drops = point_queries(ctx, pts, rr, True, k, stats=True, closest=closest)["drops"]
        assert not any(drops), "%s, %s pass: the walk drops pushes at the 64-entry cap (%s): not a case for this audit, pick another" % (name, pts.what, drops)
        for simple in kernels:
            out[pts.what, simple] = js = judge_points(tris, pts, rr, point_queries(ctx, pts, rr, simple, k, closest=closest), k)
            for j in js.values():
                assert_point_judged(j, "%s simple %d" % (name, simple), tree, capped)
    return out


# ---- through rays and aimed surfels: hit lists, occlusion, containment and signed distance -----------------------------------------------
OCC_SAMPLES, OCC_SEED = 8, 7         # occlusion over the aimed surfels: samples per surfel, a fixed seed; bias 0
CONTAIN_SAMPLES = 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _product():
    import importlib
    return importlib.import_module("raytracer-public_amd")


def through_rays(tris, k=None):
    """The aimed rays made long: each keeps its direction, its origin is moved back along the ray to where the line leaves the scene's
    bounding box grown by 5 % of its diagonal (float64, rounded to f32 before anybody sees it), t_max = +inf.  Such a ray crosses its own
    triangle at the aimed point and whatever else lies on the line.  k: rays per triangle, 4 for scenes below 1,000 triangles and 1 above.
    .aimed: the aimed rays they were made from (the surfels and near-pass points of the same audit)."""
    n = np.asarray(tris).size // 9
    k = (4 if n < 1000 else 1) if k is None else k
    a = aimed_rays(tris, k)
    V = np.asarray(tris, np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = V.min(0), V.max(0)
    pad = 0.05 * np.sqrt(((hi - lo) ** 2).sum())
    lo, hi = lo - pad, hi + pad
    o, d = a.O.astype(np.float64), a.D.astype(np.float64)
    with np.errstate(all="ignore"):
        s = np.where(d > 0, (o - lo) / d, np.where(d < 0, (o - hi) / d, np.inf)).min(1)      # o - s d reaches a face of the box
    s = np.maximum(s, 0.0)
    r = Rays()
    r.O = (o - s[:, None] * d).astype(np.float32)
    r.D = a.D
    r.t_max = np.full(len(o), np.inf, np.float32)
    r.tri, r.P, r.k, r.n, r.own, r.aimed = a.tri, a.P, k, a.n, None, a
    return r


def aimed_surfels(rays):
    """One PtSurfel record per aimed ray: p = the ray's origin, n = its direction, r_max = its t_max -- the normal points at the triangle,
    h' above it, and the sample rays end 2 h' away."""
    sf = np.zeros((len(rays.tri), 8), np.float32)
    sf[:, 0:3], sf[:, 3], sf[:, 4:7] = rays.O, rays.t_max, rays.D
    return sf


def containment_rays(points, samples=CONTAIN_SAMPLES):
    """The rays contains() counts along: the occlusion rays of the surfels {p, +inf, (0, 0, 1)}, bias 0, seed 0."""
    sf = np.zeros((len(points), 8), np.float32)
    sf[:, 0:3], sf[:, 3], sf[:, 6] = np.asarray(points, np.float32)[:, :3], np.inf, 1.0
    return _product().occlusion_rays_host(sf, samples, seed=0, bias=0.0)


PAIR_FIELDS = ("loose", "tight", "t", "u", "v", "mt", "mb")


def pair_margins(tris, rays, owner, prim):
    """margins() of the pairs (ray owner[i], triangle prim[i]), each pair evaluated once per ray set however many kernels list it."""
    keys = (np.asarray(owner, np.int64) << 32) | np.asarray(prim, np.int64)
    if getattr(rays, "pairs", None) is None:
        rays.pairs = (np.zeros(0, np.int64), {f: np.zeros(0, bool if f in ("loose", "tight") else np.float64) for f in PAIR_FIELDS})
    known_keys, memo = rays.pairs
    pos = np.minimum(np.searchsorted(known_keys, keys), max(len(known_keys) - 1, 0))
    known = known_keys[pos] == keys if len(known_keys) else np.zeros(len(keys), bool)
    new = np.unique(keys[~known])
    if len(new):
        ri = new >> 32
        m = margins(tris, rays.O[ri], rays.D[ri], new & 0xFFFFFFFF, rays.t_max[ri])
        k = np.concatenate([known_keys, new]); order = np.argsort(k, kind="stable")
        rays.pairs = known_keys, memo = k[order], {f: np.concatenate([memo[f], m[f]])[order] for f in PAIR_FIELDS}
        pos = np.searchsorted(known_keys, keys)
    return {f: memo[f][pos] for f in PAIR_FIELDS}


def judge_hits(tris, rays, lists, sorted_lists, counts):
    """lists, sorted_lists = (offsets, t, prim, u, v) of list_hits without and with sort, counts of count_hits, over the same rays (through_rays).
    O(rays + listed entries): float64 Moeller-Trumbore of each ray against its own triangle and against each listed one, nothing else.
    Lost: the own triangle is accepted with every margin to spare and is not in the list, or the count of such a ray is 0.  Phantom: an entry
    whose triangle is out of range or not even loosely accepted.  Malformed: a triangle twice; a list whose length is not the count, or not
    the sorted list's; a sorted list out of ascending (bits(t) << 32) | prim; one that is no permutation of the unsorted list (multisets of
    the four words); a t that is not positive and finite.  values_off: an entry the reference accepts for certain whose u or v is more than
    the pair's own mb, or whose t more than its mt, from float64 -- margins()' rule, 16 ulp x kappa, no new constant; .worst is the largest
    such ratio (measured over every case of tests/test_list_audit.py and tests/test_gpu_list_audit.py: at most 0.148; above 1 it is a finding
    to explain, not a margin to widen).  Nothing is excused: a list reports every crossing, so no occluder can answer in place of the own triangle."""
    t0 = time.time()
    if rays.own is None:
        rays.own = margins(tris, rays.O, rays.D, rays.tri, rays.t_max)
    aud = rays.own["tight"]
    n, R = rays.n, len(rays.tri)
    off, t, prim, u, v = [np.asarray(a) for a in lists]
    soff, st, sprim, su, sv = [np.asarray(a) for a in sorted_lists]
    off, soff = off.astype(np.int64), soff.astype(np.int64)
    for o_, p_ in ((off, prim), (soff, sprim)):
        assert len(o_) == R + 1 and o_[0] == 0 and o_[-1] == len(p_) and np.all(np.diff(o_) >= 0), "offsets are no offsets into the entries"
    lens, slens = np.diff(off), np.diff(soff)
    owner, sowner = np.repeat(np.arange(R), lens), np.repeat(np.arange(R), slens)
    phantom = np.zeros(R, bool); malformed = np.zeros(R, bool)
    # every listed entry against float64
    inr = prim < n
    phantom[owner[~inr]] = True
    ei = np.flatnonzero(inr)
    oe = owner[ei]
    m = pair_margins(tris, rays, oe, prim[ei])
    phantom[oe[~m["loose"]]] = True
    sure = m["tight"]
    with np.errstate(all="ignore"):
        ratio = np.maximum(np.maximum(np.abs(u[ei] - m["u"]), np.abs(v[ei] - m["v"])) / m["mb"], np.abs(t[ei] - m["t"]) / m["mt"])
        ratio = np.where(sure, ratio, 0.0)
        badt = ~(np.isfinite(t) & (t > 0)); sbadt = ~(np.isfinite(st) & (st > 0))
    values_off = np.unique(oe[~(ratio <= 1)])
    # form
    key = np.sort((owner << 32) | prim.astype(np.int64))
    malformed[key[1:][key[1:] == key[:-1]] >> 32] = True                       # a triangle twice in one list
    malformed |= (np.asarray(counts).astype(np.int64) != lens) | (lens != slens)
    malformed[owner[badt]] = True; malformed[sowner[sbadt]] = True
    skey = (_bits(st).astype(np.uint64) << np.uint64(32)) | sprim.astype(np.uint64)
    down = (sowner[1:] == sowner[:-1]) & (skey[1:] < skey[:-1])
    malformed[sowner[1:][down]] = True                                         # not in ascending order of (bits(t) << 32) | prim
    same = lens == slens                                                       # a permutation: the lists of equal length, as multisets of the four words
    rows = []
    for ow, (a, b, c, d_) in ((owner, (t, prim, u, v)), (sowner, (st, sprim, su, sv))):
        pick = np.flatnonzero(same[ow])
        k1 = (ow[pick] << 32) | b[pick].astype(np.int64)
        k2 = (_bits(a)[pick].astype(np.int64) << 32) | _bits(c)[pick].astype(np.int64)
        k3 = _bits(d_)[pick].astype(np.int64)
        order = np.lexsort((k3, k2, k1))
        rows.append((k1[order], k2[order], k3[order]))
    differ = (rows[0][0] != rows[1][0]) | (rows[0][1] != rows[1][1]) | (rows[0][2] != rows[1][2])
    malformed[np.unique(np.concatenate([rows[0][0][differ], rows[1][0][differ]]) >> 32)] = True
    has_own = np.isin((np.arange(R) << 32) | rays.tri, key)
    lost = aud & (~has_own | (np.asarray(counts) == 0))
    j = PointJudgement()
    j.query, j.what, j.excuse, j.n, j.R, j.tri, j.auditable = "list_hits", "through", "excused", n, R, rays.tri, aud
    j.lost, j.phantom, j.malformed, j.values_off = np.flatnonzero(lost), np.flatnonzero(phantom), np.flatnonzero(malformed), values_off
    j.excused = np.zeros(R, bool)
    j.lost_tris = np.unique(rays.tri[j.lost])
    j.share_not_auditable = float((~aud).mean()) if R else 0.0
    j.share_excused, j.entries = 0.0, len(prim)
    j.worst = float(ratio.max(initial=0.0))
    j.share_margin = float((m["loose"] & ~sure).mean()) if len(ei) else 0.0
    j.longest = int(lens.max(initial=0))
    j.sorted = (soff, st, sprim, su, sv)
    j.certain = (oe[sure], prim[ei][sure])                                      # (ray, triangle) of every entry the reference accepts for certain
    j.seconds = time.time() - t0
    return j


def occlusion_floor(tris, rays, samples=OCC_SAMPLES, seed=OCC_SEED):
    """Per aimed surfel: how many of its sample rays (occlusion_rays_host: pinned to numpy bit for bit, no part of any walk; bias 0) accept
    the surfel's own triangle with every margin to spare, in float64, against that triangle alone.  Computed once per ray set."""
    memo = getattr(rays, "occ", None)
    if memo is None or memo[0] != (samples, seed):
        sr = _product().occlusion_rays_host(aimed_surfels(rays), samples, seed=seed, bias=0.0)
        m = margins(tris, sr[:, 0:3], sr[:, 4:7], np.repeat(rays.tri, samples), sr[:, 3])
        rays.occ = memo = ((samples, seed), m["tight"].reshape(-1, samples).sum(1))
    return memo[1]


def judge_occlusion(tris, rays, result, samples=OCC_SAMPLES, seed=OCC_SEED):
    """result = (visibility, unoccluded, samples) of occlusion over aimed_surfels(rays), bias 0.  A lower bound: samples - unoccluded must
    be at least occlusion_floor -- any-hit may be answered by any triangle, but a sample ray that certainly crosses the own triangle within
    r_max is occluded.  A shortfall is a lost triangle.  Malformed: a samples field that is not `samples`, a visibility that is not the
    correctly rounded unoccluded / samples.  Not auditable: a surfel none of whose sample rays certainly crosses its triangle;
    share_blind_tris: triangles without an auditable surfel."""
    t0 = time.time()
    floor = occlusion_floor(tris, rays, samples, seed)
    vis, unocc, smp = [np.asarray(a) for a in result]
    n, R = rays.n, len(rays.tri)
    want = (unocc.astype(np.float64) / samples).astype(np.float32)
    j = PointJudgement()
    j.query, j.what, j.excuse, j.n, j.R, j.tri, j.auditable = "occlusion", "surfel", "excused", n, R, rays.tri, floor > 0
    j.lost = np.flatnonzero(samples - unocc.astype(np.int64) < floor)
    j.phantom = np.zeros(0, np.int64)
    j.malformed = np.flatnonzero((smp != samples) | (unocc > samples) | (_bits(vis) != _bits(want)))
    j.excused = np.zeros(R, bool)
    j.lost_tris = np.unique(rays.tri[j.lost])
    j.share_not_auditable = float((floor == 0).mean()) if R else 0.0
    j.share_blind_tris = float((np.bincount(rays.tri[floor > 0], minlength=n) == 0).mean()) if n else 0.0
    j.share_sure = float(floor.sum()) / max(R * samples, 1)
    j.share_excused, j.entries, j.seconds = 0.0, int(floor.sum()), time.time() - t0
    return j


def audit_lists(ctx, tris, name, kernels=KERNELS, capped=True, rays=None, brute=True, tree=None):
    """Every triangle through the hit lists, the long counting walk, containment, and (on a device context) occlusion and signed distance of
    `ctx`: one through ray per triangle (four below 1,000 triangles) through list_hits, list_hits(sort) and count_hits of every kernel in
    `kernels` and through judge_hits; OCC_SAMPLES occlusion samples per aimed surfel through judge_occlusion; and the compositions as
    equalities -- occlusion with occlusion_rays -> trace_rays(any_hit), contains(samples 3) over the near-pass points with the parity
    majority of count_hits over containment_rays, signed_distance with closest_points under contains' sign.  The counting variant of every
    query runs first and must drop nothing at the 64-entry cap.  Last, list_hits(brute_force=True) goes through judge_hits: with no tree
    nothing can be lost, so that call validates the judge (`brute`: the brute-force lists do not depend on the tree, so a caller that
    audits several trees over the same triangles may ask for them once).  -> {(query, simple or "brute"): judgement}.

    Measured on the CPU over the host twins, built and refitted after `wave` and `deform`, accel 0, 1 and 2 (tests/test_list_audit.py prints
    them; the lists of a scene are the same at every level, only the stack differs).  No ray of any case was not auditable, nothing was lost,
    unexplained or malformed, no walk dropped a push.  Listed entries, built / wave / deform; the longest list; the deepest stack of the three
    levels and states (of 64; persistent_walk's short stack is 12); entries at a margin of the reference; the largest deviation of a listed
    t, u or v from float64 as a share of that pair's own margin (mt, mb):
      soups 1, 2, 3, 4, 5 (4 rays each)   4 .. 20 / = / =                 1     2    0 %              0.050
      soups 64, 65                        267, 265 / 264, 273 / 265, 266  3     7    0 %              0.067
      soup 777                            4,719 / 4,916 / 5,016           6     14   0.040 - 0.042 %  0.101
      soup 30,000 (size 0.2)              632,993 / 676,057 / 201,318     57    31   0.035 - 0.063 %  0.148     deform is of the same soup at size 0.1
      soup 30,000, size 0.02              36,174 / 36,601 / 36,953        6     21   0.064 - 0.079 %  0.123
      dragon-class 20,000                 68,114 / 69,718 / 72,262        18    25   0.046 - 0.094 %  0.114
      sponza-class 12,000                 54,860 / 61,302 / .             32    21   0.68 - 0.73 %    0.117     wave only (test_point_audit.MOVES)
      f16 grid                            1,536 / 1,952 / 3,353           9     16   0 - 0.060 %      0.091
      coincident deck (12 triangles)      288                             6     7    0 %              0.003
    A ratio above 1 would be a finding to explain, not a margin to widen; the largest anywhere is 0.148.
    Occlusion's reference side (no tree: occlusion_floor) over the same states -- sample rays that certainly cross the own triangle / surfels
    without such a ray = triangles without such a surfel above 1,000 triangles, where each has one surfel:
      small soups 69.5 - 78.1 % / 0 %;  soup 30,000 70.2 - 71.1 % / 0.023 - 0.040 %;  size 0.02 70.2 - 71.2 % / 0.050 - 0.097 %;
      dragon-class 71.8 - 72.2 % / 0 %;  sponza-class 61.0 - 61.1 % / 0.367 %;  f16 grid 71.4 - 71.6 % / 0 %.
    On the MI355X (tests/test_gpu_list_audit.py) every case above gave the twin's figures in every category through both kernels and the
    brute-force kernel, nothing lost below the occlusion bound, and every composition held."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    thr = through_rays(tris) if rays is None else rays
    aim = thr.aimed
    device = hasattr(ctx, "occlusion")
    if tree is None:
        tree = lambda: verify_bvh4(tris, ctx.read_bvh4(), built=False)
    pts = np.concatenate([aim.O, aim.t_max[:, None]], 1)
    sf = aimed_surfels(aim)
    crays = containment_rays(pts)
    # the counting variants: nothing dropped at the cap
    seen = {}
    ctx.list_hits(thr.O, thr.D, stats=True); seen["list_hits"] = dict(ctx.stats())
    ctx.count_hits(thr.O, thr.D, stats=True); seen["count_hits"] = dict(ctx.stats())
    ctx.contains(pts, samples=CONTAIN_SAMPLES, stats=True); seen["contains"] = dict(ctx.stats())
    if device:
        ctx.occlusion(sf, OCC_SAMPLES, seed=OCC_SEED, bias=0.0, stats=True); seen["occlusion"] = dict(ctx.stats())
    drops = {q: int(s["stack_drops"]) for q, s in seen.items()}
    print("%s: deepest stack %s" % (name, {q: int(s["max_stack"]) for q, s in seen.items()}))
    assert not any(drops.values()), "%s: the walk drops pushes at the 64-entry cap (%s): not a case for this audit, pick another" % (name, drops)
    out = {}

    def hits(key, **kw):
        counts = ctx.count_hits(thr.O, thr.D, **kw)
        kw["capacity"] = int(np.asarray(counts).astype(np.int64).sum()) + 1     # room for what was counted and one more: no second pass for the total
        lists = ctx.list_hits(thr.O, thr.D, **kw)
        out["hits", key] = j = judge_hits(tris, thr, lists[:5], ctx.list_hits(thr.O, thr.D, sort=True, **kw)[:5], counts)
        what = "%s %s" % (name, "brute force" if key == "brute" else "simple %d" % key)
        print("%s list_hits: longest list %d, entries at a margin of the reference %.3f %%, worst value deviation %.3f of its margin" % (what, j.longest, 100 * j.share_margin, j.worst))
        assert_point_judged(j, what, tree, capped)
    for simple in kernels:
        hits(simple, simple=simple)
        inside = ctx.contains(pts, samples=CONTAIN_SAMPLES, simple=simple)[:3]
        odd = (np.asarray(ctx.count_hits(crays, simple=simple)).reshape(len(pts), CONTAIN_SAMPLES) & 1).sum(1).astype(np.uint32)
        assert np.array_equal(inside[1], odd) and np.array_equal(inside[0], (2 * odd > CONTAIN_SAMPLES).astype(np.uint32)) and np.all(inside[2] == CONTAIN_SAMPLES), \
            "%s simple %d: contains is not the parity majority of count_hits over its rays, first points %s" % (name, simple, np.flatnonzero(inside[1] != odd)[:10].tolist())
        if not device:
            continue
        res = ctx.occlusion(sf, OCC_SAMPLES, seed=OCC_SEED, bias=0.0, simple=simple)
        out["occlusion", simple] = j = judge_occlusion(tris, aim, res)
        print("%s simple %d occlusion: %.1f %% of the sample rays certainly cross the own triangle, triangles without such a surfel %.3f %%" % (name, simple, 100 * j.share_sure, 100 * j.share_blind_tris))
        assert_point_judged(j, "%s simple %d" % (name, simple), tree, capped)
        prim = ctx.trace_rays(ctx.occlusion_rays(sf, OCC_SAMPLES, seed=OCC_SEED, bias=0.0), any_hit=True, simple=simple)[1]
        assert np.array_equal(res[1], (np.asarray(prim) == MISS).reshape(len(sf), OCC_SAMPLES).sum(1)), "%s simple %d: occlusion is not the count over its rays through trace_rays" % (name, simple)
        sd = ctx.signed_distance(pts, samples=CONTAIN_SAMPLES, simple=simple)
        cp = ctx.closest_points(pts, simple=simple)[:4]
        assert np.array_equal(_bits(np.abs(sd[0])), _bits(cp[0])) and np.array_equal(np.signbit(sd[0]), inside[0].astype(bool)) and np.array_equal(sd[1], cp[1]) \
            and np.array_equal(_bits(sd[2]), _bits(cp[2])) and np.array_equal(_bits(sd[3]), _bits(cp[3])), "%s simple %d: signed_distance is not closest_points under contains' sign" % (name, simple)
    if brute:
        hits("brute", brute_force=True)
    return out


# ---- scenes both audit files use ------------------------------------------------------------------------------------------------------
def f16_grid(cells=16):
    """Three axis-aligned planes of cells x cells quads whose vertices are multiples of 1 / 8: exactly representable in f16, every leaf box
    two f16 steps thick in one axis, every aimed ray exactly axis-parallel.  One plane is z = 0: its leaves' boxes are [-0, 2^-24] in z
    and the flush makes that [-0, +0] in the nodes above them -- boxes of zero thickness that still contain their triangles, where the slab
    test's tmax >= tmin holds with equality (with > for >= every triangle of that plane is lost)."""
    g = np.linspace(-1.0, 1.0, cells + 1)
    a, b = np.meshgrid(g[:-1], g[:-1], indexing="ij")
    s = 2.0 / cells
    out = []
    for axis, c in ((2, 0.0), (0, 0.25), (1, 0.75)):
        q = np.zeros((cells * cells, 4, 3))
        u, w = [x for x in range(3) if x != axis]
        q[:, :, axis] = c
        for k, (du, dw) in enumerate(((0, 0), (s, 0), (s, s), (0, s))):
            q[:, k, u] = a.reshape(-1) + du; q[:, k, w] = b.reshape(-1) + dw
        out.append(q[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3, 3))
    t = np.concatenate(out).astype(np.float32)
    assert np.array_equal(t, t.astype(np.float16).astype(np.float32))
    return t.reshape(-1)


def soup(n, seed, size=0.2):
    """The soups of the build tests (tests/test_bvh_invariants.py)."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3), dtype=np.float32) * 2 - 1
    return (c + (rng.random((n, 3, 3), dtype=np.float32) - 0.5) * size).astype(np.float32).reshape(-1)


def coincident_deck(layers=3, seed=0):
    """`layers` parallel unit quads at distinct z (hitlist_cases.deck), every one of them twice, the triangles in shuffled order: a ray
    through the deck crosses two triangles at every layer with the same bits of t, so in a sorted list only `prim` orders them.  The
    smallest scene of this audit in which a sort key without `prim` shows: with one or two doubled layers the visit order of some build
    level happens to ascend in `prim` at every tie; with three (seed 0) every level has ties visited the other way round."""
    import hitlist_cases as hc
    T = hc.deck(layers, seed)[0].reshape(-1, 9)
    both = np.concatenate([T, T])
    return both[np.random.default_rng(seed).permutation(len(both))].reshape(-1)


def collapse_cluster(tris, centre, count):
    """The `count` triangles nearest to `centre`, every vertex moved to the centroid of the cluster: zero-area triangles, unhittable by the specification."""
    T = np.array(tris, np.float32).reshape(-1, 3, 3)
    d = ((T.mean(1) - np.asarray(centre, np.float32)) ** 2).sum(1)
    pick = np.argsort(d, kind="stable")[:count]
    T[pick] = T[pick].reshape(-1, 3).mean(0)
    return T.reshape(-1), pick
