// f110_geometry.h — the car boxes: get_vertices, the GJK collision test and the geometry of the
// agent ray_cast (blocked beams, a box's beam window, get_range).
#pragma once

#include <hip/hip_runtime.h>

#include "f110_math.h"
#include "f110_sincos.h"

namespace f110 {

// ------------------------------------------------------------- geometry --
F110_HD double dot2(double a0, double a1, double b0, double b1) {  // ndarray.dot of 2-vectors (BLAS)
    return fma(a1, b1, a0 * b0);
}

// get_trmtx + get_vertices, collision_models.py:218-260 -> [rl, rr, fr, fl].
F110_HD void get_vertices(double x, double y, double th, double length, double width, double v[8]) {
    double s, c;
    cr_sincos(th, s, c);
    const double px[4] = {-length / 2, -length / 2, length / 2, length / 2};
    const double py[4] = {width / 2, -width / 2, -width / 2, width / 2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = c * px[k] + ((-s) * py[k] + x);
        v[2 * k + 1] = s * px[k] + (c * py[k] + y);
    }
}

// indexOfFurthestPoint + support, collision_models.py:81-110
F110_HD void gjk_support(const double *v1, const double *v2, double d0, double d1, double &o0, double &o1) {
    int i = 0, j = 0;
    double b1 = 0, b2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double p1 = fma(v1[2 * k], d0, v1[2 * k + 1] * d1);
        double p2 = fma(v2[2 * k], -d0, v2[2 * k + 1] * -d1);
        if (k == 0 || p1 > b1) { b1 = p1; i = k; }
        if (k == 0 || p2 > b2) { b2 = p2; j = k; }
    }
    o0 = v1[2 * i] - v2[2 * j];
    o1 = v1[2 * i + 1] - v2[2 * j + 1];
}

F110_HD void triple(double a0, double a1, double b0, double b1, double c0, double c1, double &o0, double &o1) {
    double ac = dot2(a0, a1, c0, c1), bc = dot2(b0, b1, c0, c1);  // tripleProduct :52-64
    o0 = b0 * ac - a0 * bc;
    o1 = b1 * ac - a1 * bc;
}

// collision (2-D GJK), collision_models.py:113-182
F110_HD bool gjk_collision(const double *v1, const double *v2) {
    double sx[3], sy[3];
    int index = 0;
    double p10 = (((v1[0] + v1[2]) + v1[4]) + v1[6]) / 4, p11 = (((v1[1] + v1[3]) + v1[5]) + v1[7]) / 4;
    double p20 = (((v2[0] + v2[2]) + v2[4]) + v2[6]) / 4, p21 = (((v2[1] + v2[3]) + v2[5]) + v2[7]) / 4;
    double d0 = p10 - p20, d1 = p11 - p21;
    if (d0 == 0 && d1 == 0) d0 = 1.0;
    double a0, a1;
    gjk_support(v1, v2, d0, d1, a0, a1);
    sx[0] = a0;
    sy[0] = a1;
    if (dot2(d0, d1, a0, a1) <= 0) return false;
    d0 = -a0;
    d1 = -a1;
    int iter = 0;
    while (iter < 1000) {
        gjk_support(v1, v2, d0, d1, a0, a1);
        ++index;
        sx[index] = a0;
        sy[index] = a1;
        if (dot2(d0, d1, a0, a1) <= 0) return false;
        double ao0 = -a0, ao1 = -a1;
        if (index < 2) {
            double ab0 = sx[0] - a0, ab1 = sy[0] - a1;
            triple(ab0, ab1, ao0, ao1, ab0, ab1, d0, d1);
            if (sqrt(fma(d1, d1, d0 * d0)) < 1e-10) {  // perpendicular(ab)
                d0 = ab1;
                d1 = -1 * ab0;
            }
            continue;
        }
        double ab0 = sx[1] - a0, ab1 = sy[1] - a1;
        double ac0 = sx[0] - a0, ac1 = sy[0] - a1;
        double q0, q1;
        triple(ab0, ab1, ac0, ac1, ac0, ac1, q0, q1);  // acperp
        if (dot2(q0, q1, ao0, ao1) >= 0) {
            d0 = q0;
            d1 = q1;
        } else {
            triple(ac0, ac1, ab0, ab1, ab0, ab1, q0, q1);  // abperp
            if (dot2(q0, q1, ao0, ao1) < 0) return true;
            sx[0] = sx[1];
            sy[0] = sy[1];
            d0 = q0;
            d1 = q1;
        }
        sx[1] = sx[2];
        sy[1] = sy[2];
        --index;
        ++iter;
    }
    return false;
}

// RaceCar.scan_angles[k] (base_classes.py:122-126), the value f110_host_tables
// stores: computed instead of loaded (same operations, no contraction)
F110_HD double beam_angle(int k, double fov, double incr) { return -fov / 2. + (double)k * incr; }

// argmin_k |angles[k] - a| over the uniform beam grid angles[k] = -fov/2 + k*incr
// (get_blocked_view_indices, laser_models.py:310-313).  The grid is strictly
// increasing, so |angles[k]-a| is V-shaped: test the analytic guess +-2 with
// NumPy's first-minimum tie break instead of a 1080-long scan.
F110_HD int nearest_beam(int B, double fov, double incr, double a) {
    if (a != a) return 0;  // np.argmin of an all-NaN array
    double g = (a + fov / 2.0) / incr;
    int k0 = g < 0 ? 0 : (g > (double)(B - 1) ? B - 1 : (int)(g + 0.5));
    int lo = k0 - 2 < 0 ? 0 : k0 - 2;
    int hi = k0 + 2 > B - 1 ? B - 1 : k0 + 2;
    int best = lo;
    double bd = fabs(beam_angle(lo, fov, incr) - a);
    for (int k = lo + 1; k <= hi; ++k) {
        double d = fabs(beam_angle(k, fov, incr) - a);
        if (d < bd) { bd = d; best = k; }
    }
    return best;
}

// One vertex of get_blocked_view_indices (laser_models.py:282-315): the beam
// nearest to the vertex bearing, relative to ego = atan2(sin(yaw), cos(yaw)).
// phi receives the vertex bearing atan2(uy, ux) (used by box_beam_window).
F110_HD int blocked_vertex_beam(double px, double py, double ego, double vx0, double vy0, int B, double fov,
                                double incr, double &phi) {
    double vx = vx0 - px, vy = vy0 - py;
    double nrm = sqrt(vx * vx + vy * vy);
    double ux = vx / nrm, uy = vy / nrm;
    phi = atan2(uy, ux);
    double angle = ego - phi;
    if (angle > kPi) angle = angle - 2 * kPi;
    else if (angle < -kPi) angle = angle + 2 * kPi;
    return nearest_beam(B, fov, incr, -angle);
}

// get_blocked_view_indices, laser_models.py:282-315
F110_HD void blocked_range(double px, double py, double pth, const double v[8], int B, double fov, double incr,
                           int &lo, int &hi) {
    double ey, ex;
    cr_sincos(pth, ey, ex);
    double ego = atan2(ey, ex);
    int mn = 0, mx = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double vx = v[2 * i] - px, vy = v[2 * i + 1] - py;
        double nrm = sqrt(vx * vx + vy * vy);
        double ux = vx / nrm, uy = vy / nrm;
        double angle = ego - atan2(uy, ux);
        if (angle > kPi) angle = angle - 2 * kPi;
        else if (angle < -kPi) angle = angle + 2 * kPi;
        int k = nearest_beam(B, fov, incr, -angle);
        if (i == 0 || k < mn) mn = k;
        if (i == 0 || k > mx) mx = k;
    }
    lo = mn;
    hi = mx;
}

// Which beams of a ray_cast can reach an opponent's box at all.  From scan
// origin o outside the (convex) box, a ray at world angle theta meets an
// edge only if theta lies in the angular interval the box subtends at o.
// Beams more than kBeamMargin outside it miss every edge by a relative
// margin (>= 1e-9 of the edge parameter for o at least kBoxClearance away),
// far above f64 rounding, so the reference's get_range returns inf for all
// four edges and the beam can be skipped.  The filter is off (half = inf)
// when o is within kBoxClearance of a vertex or of an edge's line (which
// includes are_collinear's 1e-8 test: get_range's denom == 0 branch ignores
// the beam direction there), or inside the box.
constexpr double kBeamMargin = 1e-5;
constexpr double kBoxClearance = 1e-3;

F110_HD double wrap_pm_pi(double a) { return a - 2.0 * kPi * rint(a * (0.5 / kPi)); }  // approximate

// The beam-index ranges [r0a, r0b] and [r1a, r1b] (either may be empty) that
// can hold beams of the window (center, half) for a car at yaw oth:
// angle(b) = oth + angles[b] with angles[b] ~ -fov/2 + b*incr.  Padded by 2
// beams; callers still apply the exact per-beam window test.
F110_HD void window_beam_ranges(double oth, double fov, double incr, int B, double center, double half, int &r0a,
                                int &r0b, int &r1a, int &r1b) {
    r0a = 0;
    r0b = B - 1;
    r1a = 1;
    r1b = 0;
    if (!(half < kPi)) return;  // no filter: every beam
    // u(b) = angle(b) - (center - half), taken mod 2pi into [0, 2pi)
    double c0 = oth - fov / 2.0 - (center - half);
    c0 = c0 - 2.0 * kPi * floor(c0 * (0.5 / kPi));
    // in the window iff (c0 + b*incr) mod 2pi <= 2*half
    const double w = 2.0 * half;
    r0a = 0;
    r0b = c0 <= w ? (int)floor((w - c0) / incr) + 2 : -1;
    r1a = (int)ceil((2.0 * kPi - c0) / incr) - 2;
    r1b = (int)floor((2.0 * kPi - c0 + w) / incr) + 2;
    if (r0b > B - 1) r0b = B - 1;
    if (r1a < 0) r1a = 0;
    if (r1b > B - 1) r1b = B - 1;
    if (r1a <= r1b && r0a <= r0b && r1a <= r0b + 1) {  // overlapping: one range
        r0b = r1b > r0b ? r1b : r0b;
        r1a = 1;
        r1b = 0;
    }
}

F110_HD void box_beam_window(double ox, double oy, const double v[8], const double phi_in[4], double &center,
                             double &half) {
    center = 0.0;
    half = INFINITY;
    double phi[4];
    int inside_pos = 0, inside_neg = 0;
    for (int q = 0; q < 4; ++q) {
        const double ax = v[2 * q], ay = v[2 * q + 1];
        const double bx = v[2 * ((q + 1) & 3)], by = v[2 * ((q + 1) & 3) + 1];
        const double dx = ax - ox, dy = ay - oy;
        if (dx * dx + dy * dy < kBoxClearance * kBoxClearance) return;
        // |cross(va - o, o - vb)| = |edge| * distance(o, edge line): no filter
        // within kBoxClearance of any edge line (this also covers
        // are_collinear's 1e-8 test and keeps d1's sign robust for rays whose
        // backward half crosses an edge)
        const double c = dx * (oy - by) - dy * (ox - bx);
        const double ex = bx - ax, ey = by - ay;
        if (fabs(c) < 1e-8 || c * c < kBoxClearance * kBoxClearance * (ex * ex + ey * ey)) return;
        // side of o relative to edge a->b (all one sign: o inside the box)
        const double side = (bx - ax) * (oy - ay) - (by - ay) * (ox - ax);
        inside_pos += side > 0.0;
        inside_neg += side < 0.0;
        // bearing of the vertex from o (any approximation is fine: the margin
        // is 1e-5 rad); phi_in = the blocked-range bearings when available
        phi[q] = phi_in ? phi_in[q] : atan2(dy, dx);
    }
    if (inside_pos == 4 || inside_neg == 4) return;
    double lo = 0.0, hi = 0.0;
    for (int q = 1; q < 4; ++q) {
        const double d = wrap_pm_pi(phi[q] - phi[0]);
        lo = d < lo ? d : lo;
        hi = d > hi ? d : hi;
    }
    if (hi - lo > kPi - 1e-3) return;  // o very close to the box: no filter
    center = phi[0] + 0.5 * (lo + hi);
    half = 0.5 * (hi - lo) + kBeamMargin;
}

// get_range, laser_models.py:249-280, with the beam's (cos, sin)(theta + pi/2)
// hoisted out of the 4-edge loop (same values each call).
F110_HD double get_range(double ox, double oy, double v30, double v31, double va0, double va1, double vb0,
                         double vb1) {
    double v10 = ox - va0, v11 = oy - va1;
    double v20 = vb0 - va0, v21 = vb1 - va1;
    double denom = dot2(v20, v21, v30, v31);
    double distance = INFINITY;
    if (fabs(denom) > 0.0) {
        double d1 = (v20 * v11 - v21 * v10) / denom;
        double d2 = dot2(v10, v11, v30, v31) / denom;
        if (d1 >= 0.0 && d2 >= 0.0 && d2 <= 1.0) distance = d1;
    } else {
        double ba0 = va0 - ox, ba1 = va1 - oy;  // are_collinear(o, va, vb) :232-247
        double ca0 = ox - vb0, ca1 = oy - vb1;
        if (fabs(ba0 * ca1 - ba1 * ca0) < 1e-8) {
            double e0 = va0 - ox, e1 = va1 - oy, f0 = vb0 - ox, f1 = vb1 - oy;
            double da = sqrt(fma(e1, e1, e0 * e0));
            double db = sqrt(fma(f1, f1, f0 * f0));
            distance = da <= db ? da : db;
        }
    }
    return distance;
}

}  // namespace f110
