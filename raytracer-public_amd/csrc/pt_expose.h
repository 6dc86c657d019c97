// pt_expose.h -- "exposed" triangles: the float64 arithmetic shared by the device route (pt_expose.hip) and its host
// twin (pt_host.cpp::exposure_flags), the same expressions on both sides.
//
// The light of PT_MODE_PATH is directional and fixed, so whether any shadow ray that the megakernel can start on a triangle T can be
// occluded is a property of the scene.  T is EXPOSED when no triangle N of the scene -- T itself and its neighbours included, no
// exception by index -- has a point inside the prism swept towards the light from the slab in which T's shadow-ray origins lie, every
// set grown by the rounding errors derived in DESIGN.md.  The megakernel's shade pass adds the light term of a hit on an exposed
// triangle at once instead of tracing the ray.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define PT_EX_HD __host__ __device__ inline
#else
#define PT_EX_HD inline
#endif

namespace ptex {

constexpr double kEps32 = 5.9604644775390625e-8;      // 2^-24: the relative error of one f32 operation
constexpr double kShift = 1e-4;                       // pt_device.h::kEpsOrigin
constexpr double kCMin = 0.02;                        // smallest |n . L| of an exposed triangle
constexpr double kGate = 0.0999;                      // smallest |n . d| / |d| of a hit whose shadow ray is skipped (the kernel asks 0.1002 in f32)
constexpr double kGate2 = 0.2999;                     // the second tier's: steeper hits only, a third of the in-plane margin (the kernel asks 0.3008 in f32, the same ratio)
constexpr double kNormalTol = 1e-5;                   // largest distance of the stored f32 normal from the f64 one
constexpr double kDetMin = 9.99e-8;                   // below pt_device.h::kTriEps: a triangle whose |det| cannot reach it never accepts a shadow ray
constexpr double kKappaCap = 36.0 * kEps32 / 1e-3;    // triangles with a larger error factor go to the list every query tests (pt_expose.hip)
constexpr double kBoxGrow = 6.103515625e-5;           // 2^-14: what a live f16 box is grown by (the subnormal flush of DESIGN.md section 11)

struct Tri { double v0[3], e1[3], e2[3]; };

// launch bounds the mask was computed for: s_max >= |o - v| for every ray origin o (camera or surface point) and scene point v,
// d_max >= every |coordinate| of a hit point
struct Bounds { double s_max, d_max; };

PT_EX_HD double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PT_EX_HD void cross(const double* a, const double* b, double* c) { c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; }

// the light direction as the kernel holds it (pt_device.h::light_dir, f32 bits), a unit vector along it, and two unit vectors across it
struct Light { double L[3], Lh[3], U[3], V[3]; };
PT_EX_HD Light make_light(float lx, float ly, float lz) {
    Light g; g.L[0] = lx; g.L[1] = ly; g.L[2] = lz;
    const double il = 1.0 / sqrt(dot(g.L, g.L));
    for (int a = 0; a < 3; ++a) g.Lh[a] = g.L[a] * il;
    const double ax[3] = {1.0, 0.0, 0.0};
    double u[3]; cross(g.Lh, ax, u);
    const double iu = 1.0 / sqrt(dot(u, u));
    for (int a = 0; a < 3; ++a) g.U[a] = u[a] * iu;
    cross(g.Lh, g.U, g.V);
    return g;
}

// what a query keeps of its triangle T
struct Query {
    bool ok;
    double c, nf[3], v0s[3];        // |n . Lh|, the unit normal on the light's side, v0 shifted by kShift along it
    double p[3][2];                 // the shifted triangle's corners across the light
    double en[3][3];                // its edges as inward half-planes a u + b v + d >= 0, (a, b) a unit vector
    double rho_n, rho_xy;           // how far an origin can lie off the shifted plane, and off the shifted triangle within it (for hits at the query's gate or above)
    double sinphi;                  // the sine of the angle between its edges e1, e2 (rho_xy_at)
    double cen[3], rad;             // centre and radius of the shifted triangle
    double lo[2], hi[2], wmin;      // its bounds across the light, its smallest depth along it
};

// error factor of a triangle as an occluder: an accepted shadow-ray test puts the exact line within kappa * S of the triangle, S the
// largest operand of the test; < 0: the test can never be accepted
PT_EX_HD double kappa_of(const Tri& n, const Light& g) {
    double nn[3]; cross(n.e1, n.e2, nn);
    const double l1 = sqrt(dot(n.e1, n.e1)), l2 = sqrt(dot(n.e2, n.e2));
    double pv[3]; cross(g.L, n.e2, pv);
    const double det = fabs(dot(n.e1, pv));
    if (!(det + 5.3 * kEps32 * l1 * l2 >= kDetMin)) return -1.0;
    return 36.0 * kEps32 * l1 * l2 / det;          // det = |e1| |e2| sin(phi) |n . L|
}

// rho_xy for another gate: the one term of a query that depends on the gate.  A larger gate gives a smaller margin, so what is exposed at
// one gate is exposed at every larger one.
PT_EX_HD double rho_xy_at(const Query& q, const Bounds& b, double gate) { return 36.0 * kEps32 * b.s_max / (q.sinphi * gate) + q.rho_n; }

// gate: the smallest |n . d| / |d| of the hits whose shadow rays the flag is to cover (kGate, kGate2)
PT_EX_HD Query make_query(const Tri& t, const float n32[3], const Light& g, const Bounds& b, double gate = kGate) {
    Query q; q.ok = false;
    double nn[3]; cross(t.e1, t.e2, nn);
    const double a2 = sqrt(dot(nn, nn)), l1 = sqrt(dot(t.e1, t.e1)), l2 = sqrt(dot(t.e2, t.e2));
    if (!(a2 > 0.0) || !(a2 < 1e300)) return q;
    double nh[3] = {nn[0] / a2, nn[1] / a2, nn[2] / a2};
    const double dn[3] = {nh[0] - n32[0], nh[1] - n32[1], nh[2] - n32[2]};
    if (!(dot(dn, dn) <= kNormalTol * kNormalTol)) return q;
    const double cl = dot(nh, g.Lh);
    q.c = fabs(cl);
    if (!(q.c >= kCMin)) return q;
    const double sgn = cl < 0.0 ? -1.0 : 1.0;
    const double sinphi = a2 / (l1 * l2);
    // origin error: off the plane by the error of t along the ray's normal component (11.5 / sin phi + 2), the rounding
    // of the product d t (one more eps S_max: |d t| <= S_max), the rounding of the sum o + d t and of + nf 1e-4 (7 eps D_max); inside the plane by the errors of u, v and t over the cosine the kernel's gate leaves
    q.rho_n = kEps32 * (11.5 * b.s_max / sinphi + 3.0 * b.s_max + 7.0 * b.d_max) + 2e-9;
    q.sinphi = sinphi;
    q.rho_xy = rho_xy_at(q, b, gate);
    if (!(q.rho_n < kShift)) return q;
    double vs[3][3];
    for (int a = 0; a < 3; ++a) {
        q.nf[a] = sgn * nh[a];
        q.v0s[a] = t.v0[a] + kShift * q.nf[a];
        vs[0][a] = q.v0s[a]; vs[1][a] = q.v0s[a] + t.e1[a]; vs[2][a] = q.v0s[a] + t.e2[a];
        q.cen[a] = q.v0s[a] + (t.e1[a] + t.e2[a]) / 3.0;
    }
    q.rad = 0.0; q.wmin = 1e300;
    q.lo[0] = q.lo[1] = 1e300; q.hi[0] = q.hi[1] = -1e300;
    for (int i = 0; i < 3; ++i) {
        q.p[i][0] = dot(vs[i], g.U); q.p[i][1] = dot(vs[i], g.V);
        const double w = dot(vs[i], g.Lh);
        const double d[3] = {vs[i][0] - q.cen[0], vs[i][1] - q.cen[1], vs[i][2] - q.cen[2]};
        const double r = sqrt(dot(d, d));
        q.rad = r > q.rad ? r : q.rad; q.wmin = w < q.wmin ? w : q.wmin;
        for (int k = 0; k < 2; ++k) { q.lo[k] = q.p[i][k] < q.lo[k] ? q.p[i][k] : q.lo[k]; q.hi[k] = q.p[i][k] > q.hi[k] ? q.p[i][k] : q.hi[k]; }
    }
    const double area = (q.p[1][0] - q.p[0][0]) * (q.p[2][1] - q.p[0][1]) - (q.p[1][1] - q.p[0][1]) * (q.p[2][0] - q.p[0][0]);
    if (!(fabs(area) > 0.0)) return q;
    const double o = area > 0.0 ? 1.0 : -1.0;
    for (int i = 0; i < 3; ++i) {
        const double* a = q.p[i]; const double* c = q.p[(i + 1) % 3];
        const double ex = c[0] - a[0], ey = c[1] - a[1], il = 1.0 / sqrt(ex * ex + ey * ey);
        if (!(il < 1e300)) return q;
        q.en[i][0] = -ey * il * o; q.en[i][1] = ex * il * o;
        q.en[i][2] = -(q.en[i][0] * a[0] + q.en[i][1] * a[1]);
    }
    q.ok = true;
    return q;
}

// the largest operand of a shadow-ray test of triangle n from an origin on T: |so - v0| plus the way along the ray to n's far corner
PT_EX_HD double operand_of(const Query& q, double rho_xy, const Tri& n) {
    const double d[3] = {n.v0[0] - q.cen[0], n.v0[1] - q.cen[1], n.v0[2] - q.cen[2]};
    return sqrt(dot(d, d)) + q.rad + rho_xy + sqrt(dot(n.e1, n.e1)) + sqrt(dot(n.e2, n.e2));
}

// Does triangle n reach into T's prism?  n is clipped against the three planes through T's edges (pushed out by `grow`) that contain
// the light direction; the height over T's shifted plane along the light is affine on the clipped polygon, so its maximum is at a corner.
// rho_xy: the in-plane margin of the tier asked for (q.rho_xy, or rho_xy_at of another gate -- everything else of q is the same for every gate).
PT_EX_HD bool blocks(const Query& q, double rho_xy, const Tri& n, const Light& g) {
    const double kap = kappa_of(n, g);
    if (kap < 0.0) return false;
    const double rho_nb = kap * operand_of(q, rho_xy, n);
    const double grow = rho_xy + q.rho_n + rho_nb, hthr = -(q.rho_n + rho_nb) / q.c;
    if (!(grow < 1e300)) return true;
    double pu[8], pv[8], ph[8], qu[8], qv[8], qh[8];
    for (int i = 0; i < 3; ++i) {
        double x[3], r[3];
        for (int a = 0; a < 3; ++a) { x[a] = n.v0[a] + (i == 1 ? n.e1[a] : (i == 2 ? n.e2[a] : 0.0)); r[a] = x[a] - q.v0s[a]; }
        pu[i] = dot(x, g.U); pv[i] = dot(x, g.V); ph[i] = dot(r, q.nf) / q.c;
    }
    {   // beside T's grown footprint altogether: nothing to clip
        double lo0 = pu[0], hi0 = pu[0], lo1 = pv[0], hi1 = pv[0];
        for (int i = 1; i < 3; ++i) { lo0 = pu[i] < lo0 ? pu[i] : lo0; hi0 = pu[i] > hi0 ? pu[i] : hi0; lo1 = pv[i] < lo1 ? pv[i] : lo1; hi1 = pv[i] > hi1 ? pv[i] : hi1; }
        if (lo0 > q.hi[0] + grow || hi0 < q.lo[0] - grow || lo1 > q.hi[1] + grow || hi1 < q.lo[1] - grow) return false;
    }
    int m = 3;
    for (int e = 0; e < 3 && m > 0; ++e) {
        const double a = q.en[e][0], b = q.en[e][1], d = q.en[e][2] + grow;
        int k = 0;
        for (int i = 0; i < m; ++i) {
            const int j = i + 1 == m ? 0 : i + 1;
            const double si = a * pu[i] + b * pv[i] + d, sj = a * pu[j] + b * pv[j] + d;
            if (si >= 0.0) { qu[k] = pu[i]; qv[k] = pv[i]; qh[k] = ph[i]; ++k; }
            if ((si >= 0.0) != (sj >= 0.0)) {
                const double f = si / (si - sj);
                qu[k] = pu[i] + f * (pu[j] - pu[i]); qv[k] = pv[i] + f * (pv[j] - pv[i]); qh[k] = ph[i] + f * (ph[j] - ph[i]); ++k;
            }
        }
        m = k;
        for (int i = 0; i < m; ++i) { pu[i] = qu[i]; pv[i] = qv[i]; ph[i] = qh[i]; }
    }
    for (int i = 0; i < m; ++i) if (ph[i] > hthr) return true;
    return false;
}
PT_EX_HD bool blocks(const Query& q, const Tri& n, const Light& g) { return blocks(q, q.rho_xy, n, g); }

// Can anything inside the box [mn, mx] (a live f16 box, grown here) block T?  No when the box lies beside T's grown footprint or
// below the lowest point of its shifted plane over that footprint; the growth assumes the largest error factor a walked triangle has.
PT_EX_HD bool box_may_block(const Query& q, const double* mn, const double* mx, const Light& g) {
    double c[3], h[3];
    for (int a = 0; a < 3; ++a) { c[a] = 0.5 * (mn[a] + mx[a]); h[a] = 0.5 * fabs(mx[a] - mn[a]) + kBoxGrow; }      // (an inverted box counts as the box between its planes)
    if (!(fabs(c[0]) + fabs(c[1]) + fabs(c[2]) + h[0] + h[1] + h[2] < 1e300)) return true;      // not finite: nothing is known about it
    const double d[3] = {c[0] - q.cen[0], c[1] - q.cen[1], c[2] - q.cen[2]};
    const double diag = 2.0 * sqrt(dot(h, h));
    const double s_box = sqrt(dot(d, d)) + q.rad + q.rho_xy + 2.5 * diag;
    if (!(s_box < 1e300)) return true;
    const double rho_nb = kKappaCap * s_box, grow = q.rho_xy + q.rho_n + rho_nb;
    const double cu = dot(c, g.U), cv = dot(c, g.V), cw = dot(c, g.Lh);
    const double ru = fabs(g.U[0]) * h[0] + fabs(g.U[1]) * h[1] + fabs(g.U[2]) * h[2];
    const double rv = fabs(g.V[0]) * h[0] + fabs(g.V[1]) * h[1] + fabs(g.V[2]) * h[2];
    const double rw = fabs(g.Lh[0]) * h[0] + fabs(g.Lh[1]) * h[1] + fabs(g.Lh[2]) * h[2];
    if (cu - ru > q.hi[0] + grow || cu + ru < q.lo[0] - grow || cv - rv > q.hi[1] + grow || cv + rv < q.lo[1] - grow) return false;
    const double slope = sqrt(1.0 - q.c * q.c < 0.0 ? 0.0 : 1.0 - q.c * q.c) / q.c;
    return cw + rw >= q.wmin - grow * slope - (q.rho_n + rho_nb) / q.c;
}

} // namespace ptex
